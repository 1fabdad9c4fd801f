"""device.Workspace (the persistent, named scratch of one task), device.Scope (call-lifetime ownership) and device.FlagRing, driven
by a fake context whose `alloc` returns recording buffers: no library and no GPU."""
import pytest

from boa_hip.device import BufferView, FlagRing, Scope, Workspace


class FakeBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes, self.ptr = ctx, int(nbytes), 0x1000 * (len(ctx.allocated) + 1)
        self.frees = self.zeros = 0

    def free(self):
        self.frees += 1
        self.ctx.live.discard(self)

    def zero(self):
        self.zeros += 1


class FakeContext:
    def __init__(self):
        self.allocated, self.live = [], set()

    def alloc(self, nbytes):
        b = FakeBuffer(self, nbytes)
        self.allocated.append(b)
        self.live.add(b)
        return b


class FakeArray:
    """What Scope sees of a DevArray: `.buf` shared between views, `.free()` frees the buffer."""

    def __init__(self, buf):
        self.buf = buf

    def free(self):
        self.buf.free()


def test_buf_reuses_a_buffer_that_is_large_enough():
    ctx = FakeContext()
    ws = Workspace(ctx)
    a = ws.buf("acc", 100)
    assert ws.buf("acc", 100) is a and ws.buf("acc", 40) is a
    assert len(ctx.allocated) == 1 and a.frees == 0 and a.nbytes == 100


def test_buf_grows_by_freeing_once_and_allocating_the_asked_size():
    ctx = FakeContext()
    ws = Workspace(ctx)
    a = ws.buf("acc", 100)
    b = ws.buf("acc", 101)
    assert b is not a and a.frees == 1 and b.nbytes == 101
    assert [x.nbytes for x in ctx.allocated] == [100, 101] and ctx.live == {b}


def test_buf_never_shrinks():
    ctx = FakeContext()
    ws = Workspace(ctx)
    ws.buf("acc", 10)
    b = ws.buf("acc", 200)
    assert ws.buf("acc", 10) is b and ws.buf("acc", 200) is b
    assert b.nbytes == 200 and b.frees == 0 and len(ctx.allocated) == 2


def test_names_are_independent():
    ctx = FakeContext()
    ws = Workspace(ctx)
    a, n = ws.buf("acc", 64), ws.buf("n", 8)
    assert a is not n and ws.buf("acc", 64) is a and ws.buf("n", 8) is n
    ws.buf("n", 16)
    assert a.frees == 0 and n.frees == 1


def test_init_runs_on_first_allocation_and_on_growth_only():
    ctx = FakeContext()
    ws = Workspace(ctx)
    seen = []
    a = ws.buf("ones", 32, init=seen.append)
    assert seen == [a]
    assert ws.buf("ones", 32, init=seen.append) is a and ws.buf("ones", 8, init=seen.append) is a
    assert seen == [a]
    b = ws.buf("ones", 64, init=seen.append)
    assert seen == [a, b] and b.nbytes == 64


def test_turn_alternates_per_name():
    ws = Workspace(FakeContext())
    assert [ws.turn("job") for _ in range(3)] == [0, 1, 0]
    assert ws.turn("seq") == 0          # a second name starts at 0 ...
    assert ws.turn("job") == 1          # ... and does not advance the first
    assert [ws.turn("seq") for _ in range(2)] == [1, 0]
    assert not ws._bufs                 # counters are not buffers


def test_flag_with_a_ring_hands_out_consecutive_slots_and_allocates_nothing():
    ctx = FakeContext()
    ws = Workspace(ctx, ring=True)
    ring = ws.ring
    assert isinstance(ring, FlagRing) and ws.ring is ring
    assert [b.nbytes for b in ctx.allocated] == [4 * FlagRing.SLOTS] and ring.buf.zeros == 1
    flags = [ws.flag() for _ in range(3)]
    assert len(ctx.allocated) == 1
    assert all(isinstance(f, BufferView) and f.nbytes == 4 for f in flags)
    assert [f.ptr - ring.buf.ptr for f in flags] == [0, 4, 8] and ring.n == 3
    ring.reset()
    assert ring.n == 0 and ring.buf.zeros == 2
    assert ws.flag().ptr == ring.buf.ptr


def test_flag_without_a_ring_is_one_zeroed_buffer():
    ctx = FakeContext()
    ws = Workspace(ctx)
    assert ws.ring is None
    f = ws.flag()
    assert f.nbytes == 4 and f.zeros == 1
    assert ws.flag() is f and f.zeros == 2 and len(ctx.allocated) == 1


def test_free_releases_everything_and_may_be_called_twice():
    ctx = FakeContext()
    ws = Workspace(ctx, ring=True)
    ws.buf("acc", 100), ws.buf("n", 10), ws.flag()
    ws.buf("acc", 200)
    assert len(ctx.live) == 3
    ws.free()
    assert not ctx.live
    ws.free()
    assert all(b.frees == 1 for b in ctx.allocated)
    assert ws.buf("acc", 10).nbytes == 10 and len(ctx.live) == 1      # usable again: nothing stale is handed out
    ws.free()
    assert not ctx.live


def test_leaving_the_with_block_by_an_exception_frees_everything():
    ctx = FakeContext()
    with pytest.raises(ValueError):
        with Workspace(ctx, ring=True) as ws:
            ws.buf("acc", 100)
            ws.flag()
            raise ValueError("boom")
    assert len(ctx.allocated) == 2 and not ctx.live


def test_scope_frees_two_views_of_one_buffer_once():
    ctx = FakeContext()
    with Scope() as sc:
        buf = ctx.alloc(64)
        a = sc.own(FakeArray(buf))
        assert sc.own(FakeArray(buf)) is not a
        raw = sc.own(ctx.alloc(8))          # a bare buffer is its own owner
    assert buf.frees == 1 and raw.frees == 1 and not ctx.live


def test_scope_keeps_what_was_released():
    ctx = FakeContext()
    with Scope() as sc:
        kept, gone = ctx.alloc(64), ctx.alloc(64)
        sc.own(FakeArray(kept))
        view = sc.own(FakeArray(kept))
        sc.own(FakeArray(gone))
        assert sc.release(view) is view      # every recorded object sharing the buffer is forgotten
    assert kept.frees == 0 and gone.frees == 1 and ctx.live == {kept}


def test_scope_frees_the_rest_when_the_block_raises():
    ctx = FakeContext()
    with pytest.raises(KeyError):
        with Scope() as sc:
            a = sc.own(FakeArray(ctx.alloc(4)))
            b = sc.own(FakeArray(ctx.alloc(4)))
            sc.release(b)
            raise KeyError("boom")
    assert a.buf.frees == 1 and b.buf.frees == 0


def test_a_full_ring_checks_itself():
    """64 slots in use: the 65th `next` reads the ring first (FlagRing.check), which needs the real download -- here it must at
    least be attempted on the ring's buffer, after which slot 0 is handed out again."""
    ctx = FakeContext()
    ring = FlagRing(ctx)
    calls = []
    ring.check = lambda: (calls.append(ring.n), setattr(ring, "n", 0))
    for _ in range(FlagRing.SLOTS):
        ring.next()
    assert calls == [] and ring.n == FlagRing.SLOTS
    assert ring.next().ptr == ring.buf.ptr and calls == [FlagRing.SLOTS] and ring.n == 1

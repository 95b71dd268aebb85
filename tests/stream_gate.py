"""Late inputs on a non-blocking stream, for tests of the C ABI's stream contract (include/btlbf.h: a BTLBF_DEVICE call
reads its inputs and writes its outputs in the order of `stream`).

On torch's default stream -- the legacy NULL stream, which waits for every blocking stream -- and with inputs that were
settled long before the call, a kernel launched on stream 0 instead of `s`, a blocking copy that reads a caller's array
before the caller's stream has produced it, or a result finished on a side stream and never joined back all give the
right answer.  Here the call is issued on a torch side stream (created non-blocking, what `with torch.cuda.stream(s):`
gives a user) while its inputs are still IN FLIGHT on that stream:

    delay = calibrate()               once per module: the delay, measured, and the stream of every gate (pick_stream)
    g = Gate(delay, ms, reg)          one non-blocking stream g.s; reg: the poison.Poison registry of the outputs
    dst = g.late(dst, real, decoy)    dst holds `decoy` now and `real` only after a delay queued on g.s
    out, ptr = g.alloc(shape, dtype)  a poisoned, guarded output, filled on g.s BEFORE the delay
    g.arm()                           decoys written, device synchronised; then on g.s: the delay, the copies of every
                                      `real`, the event g.opened
    g.in_flight()                     g.opened has not completed: the precondition of every case
    g.collect(outs)                   clone() of every output and of every guarded allocation on g.s, g.s.synchronize()
                                      and NOTHING WIDER, guards checked on the clones -> host copies of the outputs

A decoy is always a VALID input of the same shape (other reads, another ascending `starts` with the same ends, other ids
below n_ids, other hash rows): a library that reads too early gives a wrong answer or an error code, never an access
out of range.  Nothing here waits on host memory, calls back into the host or blocks a queue on a value: the delay is a
kernel that ends by itself (torch.cuda._sleep) or, where that does not delay, a chain of in-place passes over a large
tensor, calibrated once with HIP events (calibrate()).  If the test process dies, the queue drains.

run_gated() is the shape of a case: once with settled inputs (the host time of the call is measured, and the same check
shows that the case is right when nothing is late), then with late inputs; a case whose gate had opened before the call
was issued -- the host stalled -- is set up once more with four times the delay, and fails if that does not help: no
case passes without having met the precondition.  No GPU test of its own; tests/test_gpu_stream_order.py uses it."""
import time

import numpy as np

import poison

DELAY_MS = 50.0  # a tuning value: long against the host time of a call (REPORT), short against a test's budget


class Delay:
    """a delay of about `ms` milliseconds queued on the current stream; what one unit costs is measured, not assumed"""

    def __init__(self, kind, per_ms, tensor=None):
        self.kind, self.per_ms, self.tensor = kind, per_ms, tensor
        self.measured_ms = None  # of DELAY_MS, with HIP events (calibrate)
        self.stream = None       # the stream of every gate (pick_stream), and what a blocking NULL-stream copy waited
        self.null_copy_ms = None  # beside a 10 ms delay on it

    def enqueue(self, ms):
        import torch

        n = max(int(self.per_ms * ms), 1)
        if self.kind == "sleep":
            torch.cuda._sleep(n)
        else:
            for _ in range(n):
                self.tensor.add_(1)


def _timed(fn):
    """milliseconds of what fn() queues on a fresh side stream, by HIP events"""
    import torch

    s = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        e0.record(s)
        fn()
        e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def calibrate(target_ms=DELAY_MS):
    """-> Delay.  torch.cuda._sleep(cycles) where it delays (its clock is whatever the device counts: the cycles per
    millisecond are measured); else element-wise passes over 256 MiB"""
    import torch

    probe = 20_000_000
    _timed(lambda: torch.cuda._sleep(1000))  # the first launch of the kernel is not what a later one costs
    ms = _timed(lambda: torch.cuda._sleep(probe))
    if ms >= 1.0:
        d = Delay("sleep", probe / ms)
    else:
        t = torch.zeros(64 << 20, dtype=torch.int32, device="cuda")
        t.add_(1)
        ms = _timed(lambda: [t.add_(1) for _ in range(16)])
        d = Delay("passes", 16 / ms, t)
    d.measured_ms = _timed(lambda: d.enqueue(target_ms))
    assert d.measured_ms >= 0.5 * target_ms, "the gate's delay of %.1f ms measures %.2f ms (%s)" % (target_ms, d.measured_ms, d.kind)
    pick_stream(d)
    return d


def pick_stream(d, tries=32):
    """The runtime multiplexes its streams over a few hardware queues, and two streams that share one run in order
    whatever their flags say: behind a delay on such a stream a blocking copy on the NULL stream waits like a copy on the
    stream itself, and the mistake these tests are after gives the right answer.  Take the first of torch's side streams
    beside whose delay of 10 ms a blocking NULL-stream copy returns at once -- in under 2 ms: a copy of 1 KiB takes some
    tens of microseconds, one that waited takes the 10 ms -- and keep it for every gate.  torch hands its side streams out
    of a pool of 32; if none of them qualifies the tests would be blind to the mistake they exist for, so that fails."""
    import torch

    x = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    x.cpu()
    for _ in range(tries):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            d.enqueue(10.0)
        t0 = time.perf_counter()
        x.cpu()  # on the NULL stream
        d.stream, d.null_copy_ms = s, (time.perf_counter() - t0) * 1e3
        s.synchronize()
        if d.null_copy_ms < 2.0:
            return
    raise AssertionError("the test would not test: beside a 10 ms delay on each of %d side streams a blocking copy on the NULL "
                         "stream took %.2f ms or more -- every side stream runs in order with the NULL stream here"
                         % (tries, d.null_copy_ms))


def to_device(a):
    """a settled device copy of a numpy array (uint64 as torch's int64); a device tensor is taken as it is"""
    import torch

    if not isinstance(a, np.ndarray):
        return a
    a = np.array(a)  # (a copy: the source may be a read-only view of bytes)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


class Gate:
    def __init__(self, delay, ms, reg=None, settled=False):
        import torch

        self.s = delay.stream or torch.cuda.Stream()  # non-blocking, as every torch side stream
        self.delay, self.ms, self.reg, self.settled = delay, ms, reg, settled
        self.lates = []
        self.opened = None

    def late(self, dst, real, decoy):
        """dst (a device tensor the library will read; None: one is made) holds `decoy` until the gate opens"""
        import torch

        real, decoy = to_device(real), to_device(decoy)
        assert real.shape == decoy.shape and real.dtype == decoy.dtype, "a decoy has the shape and type of the input"
        if dst is None:
            dst = torch.empty_like(real)
        assert dst.is_contiguous() and dst.shape == real.shape and dst.dtype == real.dtype
        self.lates.append((dst, real, decoy))
        return dst

    def alloc(self, shape, dtype, name=None):
        """a poisoned, guarded device output; call it before arm(): it is filled on g.s before the delay"""
        import torch

        assert self.opened is None, "alloc() after arm(): the fill would be queued behind the delay"
        with torch.cuda.stream(self.s):
            return self.reg.alloc(shape, dtype, device="cuda", name=name)

    def arm(self):
        import torch

        for dst, real, decoy in self.lates:
            dst.copy_(real if self.settled else decoy)
        torch.cuda.synchronize()
        with torch.cuda.stream(self.s):
            if not self.settled:
                self.delay.enqueue(self.ms)
                for dst, real, _ in self.lates:
                    dst.copy_(real, non_blocking=True)
            self.opened = torch.cuda.Event()
            self.opened.record(self.s)

    def in_flight(self):
        return not self.opened.query()

    def snapshot(self, outs):
        """a BTLBF_HOST call has returned: its numpy outputs and their guard bands as they are NOW, before anything is
        waited for -> (copies of the outputs, copies of the guarded allocations, for collect)"""
        allocs = [(name, raw.copy() if isinstance(raw, np.ndarray) else raw, nbytes) for name, raw, nbytes in (self.reg.allocs if self.reg else [])]
        return [o.copy() if isinstance(o, np.ndarray) else o for o in outs], allocs

    def collect(self, outs, allocs=None):
        """the consumer: queued on g.s after the call, it must see every output.  -> host copies (None stays None)"""
        import torch

        if allocs is None:
            allocs = self.reg.allocs if self.reg else []
        with torch.cuda.stream(self.s):
            clones = [o.clone() if isinstance(o, torch.Tensor) else o for o in outs]
            raws = [(name, raw.clone() if isinstance(raw, torch.Tensor) else raw, nbytes) for name, raw, nbytes in allocs]
        self.s.synchronize()
        shadow = poison.Poison(self.reg.byte if self.reg else 0)
        shadow.allocs = [(name, raw.cpu().numpy() if isinstance(raw, torch.Tensor) else raw, nbytes) for name, raw, nbytes in raws]
        shadow.check_guards()  # (host arrays only: it does not synchronise the device)
        return [c.cpu().numpy() if isinstance(c, torch.Tensor) else c for c in clones]


REPORT = {}  # case name -> (host milliseconds of the call with settled inputs, the call returned before the gate opened)


def run_gated(name, delay, setup, check, monkeypatch=None, byte=None, host_call=False):
    """One case.  setup(g) registers the late inputs of a fresh call and returns call, or (call, post); call() makes the
    ONE library call (production idiom: g.s is torch's current stream) and returns its outputs; post(), if given, runs
    after g.s has been synchronised (a filter body the call changed has no output to clone: it is read there).
    check(host outputs + post's values, note) asserts.  host_call: a BTLBF_HOST call -- the header says it synchronises
    before returning, so the gate must have opened when it returns, and its numpy outputs are complete then: they are
    copied the moment the call returns, before the test waits for anything, and the copies are what is checked."""
    import pytest
    import torch

    for mode, mult in (("settled", 0), ("late", 1), ("late", 4)):
        reg = poison.poisoned_outputs(monkeypatch, byte) if monkeypatch is not None else None
        g = Gate(delay, DELAY_MS * mult, reg, settled=mode == "settled")
        with torch.cuda.stream(g.s):
            made = setup(g)
            call, post = made if isinstance(made, tuple) else (made, None)
            g.arm()
            if mode == "late" and not g.in_flight():
                print("%s: the gate of %.0f ms had opened before the call was issued (the host stalled)" % (name, g.ms))
                torch.cuda.synchronize()
                continue
            t0 = time.perf_counter()
            outs = call()
            ms = (time.perf_counter() - t0) * 1e3
            early = g.in_flight()
            if host_call and mode == "late":
                assert not early, "%s: a BTLBF_HOST call returned while its stream had not reached the call" % name
            outs = [] if outs is None else list(outs) if isinstance(outs, (tuple, list)) else [outs]
            got = g.collect(*g.snapshot(outs)) if host_call else g.collect(outs)
            if post is not None:
                extra = post()
                got += list(extra) if isinstance(extra, (tuple, list)) else [extra]
        note = "%s, %s inputs; the call returned %s the gate opened" % (name, mode, "BEFORE" if early else "after")
        check(got, note)
        if mode == "settled":
            REPORT[name] = [ms, None]
            continue
        REPORT[name][1] = early
        print("STREAM_GATE %s settled_call_ms=%.3f delay_ms=%.0f returned_before_open=%s" % (name, REPORT[name][0], g.ms, early))
        return
    pytest.fail("%s: the test did not test -- the gate had opened before the call was issued, also with a delay of %.0f ms"
                % (name, 4 * DELAY_MS))

"""Stream-order harness of tests/test_gpu_streams.py: every entry of include/mythos_hip.h that takes a stream, sets a
table or reads one back is run on a stream of its own - never the null stream, on which every blocking copy, memset and
synchronisation of the library is ordered with every kernel by accident - in an order that is forced, not raced.

The delay.  ``arm(stream)`` queues ``torch.cuda._sleep`` for DELAY_MS = 50 ms on the stream (a spin on the device's clock:
plain finite work, nothing waits on a flag) and returns an event recorded right behind it.  The cycle count is calibrated
once per process against HIP events and capped so that one delay never exceeds MAX_DELAY_MS = 200 ms.  Work queued behind
the delay cannot start before the delay has run out, while the host is back at once: a host read, a blocking null-stream
copy or a launch on another stream that does not wait for the stream sees the state BEFORE that work.  The validity
condition of a case is that the event is still pending (``event.query()`` is False) straight after an entry documented as
asynchronous returns - for an entry documented to synchronise, straight BEFORE it is called, and the delay is armed again
behind it.

    delay used: 50 ms on the MI355X (calibrated per process; a call that waits for it returns after 50.2 - 50.3 ms)
    slowest covered asynchronous case, host time of its calls behind the delay against the same calls on the default
    stream (printed by every case of tests/test_gpu_streams.py): 0.65 ms against 0.14 ms; the first call of a process
    takes 3 - 8 ms on either stream (code objects, first allocations), which the reference runs on the default stream
    absorb before any delay is armed.
    The delay must stay at least 20 x that host time (here: 13 ms), or a slow host could see the delay run out before
    the assertion - the case would then report an invalid scenario, never a wrong pass.

Benign decoys.  Every device input of a case exists twice, a valid set A and a different valid set B (another frame of the
same golden trajectory, another pair list, another parameter vector).  The device buffer holds B; ``buf.copy_(A)`` is
queued behind the delay and the entry is called behind that.  A mis-ordered read therefore computes a valid answer - the
one of B - and never touches memory it should not.  Expected values are the same scenario on the default stream with A and
with B; a case first asserts that the two differ, then that the delayed-stream result is A's.

Hazard kinds (the table of tests/test_gpu_streams.py names the kinds of every case):
    IN   inputs arrive on the stream behind the delay
    OUT  outputs are consumed by a torch op on the same stream with no host synchronisation in between and are compared
         only after ``stream.synchronize()``
    SET  a launch with state A queued behind the delay, the setter with state B from the host, a second launch: the
         first result must be A's, the second B's
    GET  a getter that hands data to the host, called straight after work was queued behind the delay
"""

from __future__ import annotations

import contextlib
import functools
import time

import numpy as np
import torch

DELAY_MS = 50.0
MAX_DELAY_MS = 200.0
IN, OUT, SET, GET = "IN", "OUT", "SET", "GET"

HOST_MS = {}  # case id -> (host ms of the covered calls on the delayed stream, on the default stream): printed by the tests


@functools.lru_cache(maxsize=None)
def _cycles_per_ms() -> float:
    """Cycles of ``torch.cuda._sleep`` per millisecond, measured with events on the current device: the count is doubled
    from 1e5 until a sleep lasts at least 2 ms (at most 2^10 x 1e5 cycles, well under a second at any clock)."""
    cycles = 100_000
    for _ in range(11):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        torch.cuda._sleep(cycles)
        b.record()
        b.synchronize()
        ms = a.elapsed_time(b)
        if ms >= 2.0:
            return cycles / ms
        cycles *= 2
    raise AssertionError("torch.cuda._sleep does not delay a stream on this device")


def delay_cycles(ms: float = DELAY_MS) -> int:
    return int(_cycles_per_ms() * min(float(ms), MAX_DELAY_MS))


@contextlib.contextmanager
def delayed_stream():
    """A fresh ``torch.cuda.Stream()`` (torch creates it non-blocking: the null stream does not wait for it), made current
    for the block, and synchronised when the block ends - also when an assertion ends it."""
    _cycles_per_ms()  # (calibrated on the default stream, before anything is queued on the new one)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    try:
        with torch.cuda.stream(s):
            yield s
    finally:
        s.synchronize()


def arm(stream: torch.cuda.Stream, ms: float = DELAY_MS) -> torch.cuda.Event:
    """Queue the delay on ``stream``; -> the event recorded right behind it (pending while the delay runs)."""
    with torch.cuda.stream(stream):
        torch.cuda._sleep(delay_cycles(ms))
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev


def pending(ev: torch.cuda.Event) -> bool:
    return not ev.query()


# ---- results as flat dicts of host-comparable tensors ------------------------------------------------------------------
def flat(value, prefix="out") -> dict:
    """Any nest of tensors, arrays, numbers, dicts, tuples and Nones -> {path: tensor}; device tensors stay on the device."""
    out = {}
    if value is None:
        return out
    if isinstance(value, torch.Tensor):
        out[prefix] = value
    elif isinstance(value, np.ndarray):
        out[prefix] = torch.from_numpy(np.ascontiguousarray(value))
    elif isinstance(value, (bool, int, float, np.integer, np.floating)):
        out[prefix] = torch.tensor(value)
    elif isinstance(value, dict):
        for k in value:
            out.update(flat(value[k], f"{prefix}.{k}"))
    elif isinstance(value, (tuple, list)):
        for k, v in enumerate(value):
            out.update(flat(v, f"{prefix}[{k}]"))
    elif hasattr(value, "__dataclass_fields__"):
        for k in value.__dataclass_fields__:
            out.update(flat(getattr(value, k), f"{prefix}.{k}"))
    else:
        raise TypeError(f"{prefix}: {type(value).__name__} is not a result this harness compares")
    return out


def consume(res: dict) -> dict:
    """The OUT hazard: every device tensor of a result goes through a torch op (a copy) on the CURRENT stream, with no host
    synchronisation; host values pass through."""
    return {k: (v.clone() if v.is_cuda else v) for k, v in res.items()}


def to_host(res: dict) -> dict:
    return {k: v.detach().cpu() for k, v in res.items()}


def bit_equal(x: torch.Tensor, y: torch.Tensor) -> bool:
    """The same bytes (a NaN equals the same NaN, which torch.equal denies)."""
    if x.shape != y.shape or x.dtype != y.dtype:
        return False
    if x.numel() == 0:
        return True
    return torch.equal(x.reshape(-1).contiguous().view(torch.uint8), y.reshape(-1).contiguous().view(torch.uint8))


def same(a: dict, b: dict, close=None) -> bool:
    """Bitwise (torch.equal) on every entry; ``close`` = {key prefix: fn(a, b) -> bool} for the entries whose entry point
    is documented as equal to rounding only."""
    if a.keys() != b.keys():
        return False
    for k in a:
        fn = next((f for p, f in (close or {}).items() if k.startswith(p)), None)
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            return False
        if not (fn(x, y) if fn else bit_equal(x, y)):
            return False
    return True


def differ(a: dict, b: dict) -> bool:
    """Some entry of the two results differs bit for bit: the case has power."""
    return a.keys() == b.keys() and any(not bit_equal(a[k], b[k]) for k in a)


def describe(a: dict, b: dict) -> str:
    bad = [k for k in a if k not in b or not bit_equal(a[k], b[k])]
    return f"entries that differ: {bad[:6]}"


class Timer:
    """Host time of the covered calls of one scenario."""

    def __init__(self):
        self.ms = 0.0

    @contextlib.contextmanager
    def __call__(self):
        t = time.perf_counter()
        try:
            yield
        finally:
            self.ms += 1e3 * (time.perf_counter() - t)




# ---- a case and the probe its scenario places ---------------------------------------------------------------------------
class Probe:
    """What a case's ``call`` uses to state where the delay must still be pending.  On the default stream (``stream`` None)
    every method is a no-op, so one ``call`` serves the reference runs and the delayed run.

        out = entry(...); probe.after()                  an entry documented as asynchronous
        probe.before(); out = entry(...); probe.rearm()  an entry documented to synchronise
    """

    def __init__(self, stream=None, event=None):
        self.stream, self.event, self.checks = stream, event, 0

    def _pending(self, why: str) -> None:
        if self.stream is not None:
            assert pending(self.event), why
            self.checks += 1

    def after(self) -> None:
        self._pending("the delay ran out, or the entry synchronised although it is documented as asynchronous")

    def before(self) -> None:
        self._pending("the delay ran out before the call: the scenario proves nothing")

    def rearm(self) -> None:
        if self.stream is not None:
            self.event = arm(self.stream)


class Case:
    """One line of the table of tests/test_gpu_streams.py.

    covers    {C export: kinds} - what tests/test_stream_cases_cpu.py reads
    setup()   -> ctx: handles made on the default stream, in a state that does not depend on the scenario
    inputs(ctx) -> {"A": {name: device tensor}, "B": {...}}: the two valid input sets
    call(ctx, bufs, probe) -> any nest of tensors / arrays / numbers: the entries under test on the CURRENT stream
    install(ctx, which)    SET cases: the setter with state "A" | "B"
    check_default(ctx)     asserted after the default-stream run with A (the scenario is the one intended)
    close     {result key prefix: fn(a, b) -> bool}: entries compared to rounding, with the existing test the bound is from
    """

    def __init__(self, name, covers, setup, inputs, call, install=None, check_default=None, close=None, note=""):
        self.name, self.covers, self.setup, self.inputs, self.call = name, covers, setup, inputs, call
        self.install, self.check_default, self.close, self.note = install, check_default, close, note

    @property
    def kinds(self) -> set:
        return {k for ks in self.covers.values() for k in ks}

    def __repr__(self):
        return self.name


def _default_run(case, which: str):
    ctx = case.setup()
    bufs = {k: v.clone() for k, v in case.inputs(ctx)[which].items()}
    timer = Timer()
    with timer():
        res = flat(case.call(ctx, bufs, Probe()))
    torch.cuda.synchronize()
    if which == "A" and case.check_default is not None:
        case.check_default(ctx)
    return to_host(res), timer.ms


def in_out(case) -> None:
    """IN / OUT / GET: the buffers hold B, A is copied in behind the delay, the entries are called behind that, their
    outputs go through a torch op on the stream, and everything is compared after the stream has been synchronised."""
    (ref_a, host_default), (ref_b, _) = _default_run(case, "A"), _default_run(case, "B")
    assert differ(ref_a, ref_b), "the two input sets give the same result: the case has no power"
    ctx = case.setup()
    sets = case.inputs(ctx)
    bufs = {k: v.clone() for k, v in sets["B"].items()}
    timer = Timer()
    with delayed_stream() as s:
        probe = Probe(s, arm(s))
        for k in bufs:
            bufs[k].copy_(sets["A"][k])
        with timer():
            res = flat(case.call(ctx, bufs, probe))
        got = consume(res)
        s.synchronize()
    got = to_host(got)
    HOST_MS[case.name] = (timer.ms, host_default)
    assert probe.checks >= 1, "the case never asserted that its delay was pending"
    assert not same(got, ref_b, case.close), "the entry read its inputs before the stream delivered them: it returned the result of the decoy set B"
    assert same(got, ref_a, case.close), "the delayed-stream result is neither A's nor B's; " + describe(got, ref_a)


def set_hazard(case) -> None:
    """SET: state A installed, a launch queued behind the delay, the setter with state B from the host, a second launch.
    The first launch must see A whole, the second B.  The expected values are the same sequence on the default stream."""
    ctx = case.setup()
    case.install(ctx, "A")
    src = case.inputs(ctx)
    bufs = {k: v.clone() for k, v in src["A"].items()}
    ref_a = to_host(flat(case.call(ctx, bufs, Probe())))
    case.install(ctx, "B")
    bufs = {k: v.clone() for k, v in src["A"].items()}
    ref_b = to_host(flat(case.call(ctx, bufs, Probe())))
    torch.cuda.synchronize()
    assert differ(ref_a, ref_b), "the two states give the same result: the case has no power"
    ctx = case.setup()
    case.install(ctx, "A")
    sets = case.inputs(ctx)
    bufs = {k: v.clone() for k, v in sets["B"].items()}
    bufs2 = {k: v.clone() for k, v in sets["A"].items()}
    timer = Timer()
    with delayed_stream() as s:
        probe = Probe(s, arm(s))
        for k in bufs:
            bufs[k].copy_(sets["A"][k])
        with timer():
            first = flat(case.call(ctx, bufs, probe))
        first = consume(first)
        case.install(ctx, "B")  # from the host, while the first launch is still queued
        second = consume(flat(case.call(ctx, bufs2, Probe())))
        s.synchronize()
    first, second = to_host(first), to_host(second)
    HOST_MS[case.name] = (timer.ms, float("nan"))
    assert probe.checks >= 1, "the case never asserted that its delay was pending"
    assert not same(first, ref_b, case.close), "the setter replaced the state under a launch that was queued before it: " \
        "the first launch returned the result of state B"
    assert same(first, ref_a, case.close), "first launch: " + describe(first, ref_a)
    assert same(second, ref_b, case.close), "second launch: " + describe(second, ref_b)

"""GPU: the stream contract of every asynchronous entry point, row by row of tests/stream_cases.py.

include/bodyfit.h says "asynchronous on `stream`" and "no host synchronisation" in some sixty places and the torch layer says
"everything runs on torch.cuda.current_stream()"; the element-by-element tests all run on torch's default stream (the legacy
NULL stream), where a launch on the wrong stream, a clear on the NULL stream or a stray hipStreamSynchronize changes nothing.
Here every row runs on a SIDE stream (torch's are non-blocking: not ordered against the NULL stream) that is kept busy first.

The delay: torch.cuda._sleep (a chain of matmuls where torch has none), sized once per module with a pair of events to about
50 ms and asserted to be at least 20 ms: a busy stream, not a hang, and the only deliberate wait in this file.

(a) late inputs.  The row's inputs are twins that hold STALE BUT VALID data (another pose, another mask, other in-range ids)
    when the call is made; the real data arrives by copies enqueued on the side stream BEHIND the delay.  Whatever the call
    issues on another stream than the caller's, and whatever it reads on the host, sees the stale data and gives another number
    (never a fault: the stale inputs are legal inputs).  The result must equal the default-stream result bit for bit; that the
    two default-stream runs agree bit for bit (the documented determinism) and that the stale data alone gives ANOTHER result are
    asserted first, so a failure belongs to the stream and the check is known to be able to fail.
(b) the asynchrony promise, in the same pass.  A row whose documentation promises no host synchronisation must have returned
    while the delay was still running (the event recorded behind the input copies is not yet complete).  The warm runs of (a)
    have grown every kept workspace, so the "a growth synchronises the device once" clauses do not fire.  A row with a
    documented synchronisation prints what it did and asserts nothing.
(c) first use while the DEFAULT stream is busy, for the rows with lazily created state (the SMPL VJP and JVP with and without
    offsets, FitObjective, one row per handle kind): a fresh problem / handle, CREATED before anything else (creating one copies
    and waits on the NULL stream, which would drain the delay) after a same-sized one was run and destroyed so that the
    allocator's memory is not zero where that can be arranged; then the delay on the default stream; then the first call on
    the side stream, which makes the problem's VJP / JVP buffers or the handle's workspace; then, after a device
    synchronisation, a second call.  That the default stream was still busy when the first call had run is asserted (none of
    these first uses synchronises the device: a workspace grown from nothing is allocated, not freed).  Both must equal the default-stream result: a first-use
    clear on the NULL stream would be unordered against the kernels that write and read the cleared buffers, and one that
    landed late would wipe state the second call relies on.  THIS CHECK CAN PASS BY LUCK where such a bug exists: fresh device
    memory is often zero, a late clear of zeros changes nothing, and a clear hurts only if it lands between the kernel that
    writes a buffer and the kernel that reads it.  Before the clears of the VJP / JVP buffers were moved to the caller's stream
    (hipMemsetAsync in vjp_problem_ready / jvp_problem_ready) it passed on the MI355X in just that way: every VJP and JVP call
    rewrites what it reads of those buffers, so a clear that landed after the first call and before the second wiped nothing
    that was still needed.

The side stream.  Streams can share a hardware queue, and work on one of them is then held up behind the other's: a launch on
the NULL stream would wait for the side stream's delay like a launch on the side stream, and (a) and (c) would see nothing (with
four hardware queues every fourth of torch's streams shared the NULL stream's, and a layer mutated to launch on stream 0 passed
(a) on exactly those).  So the module picks, once, a stream that DEMONSTRABLY runs beside the default stream: an event recorded on the
default stream completes while an event behind a tenth of the delay on the side stream has not (no clock is read).

Calibration on the MI355X, with the library of the commit before the clears moved: the delay measured
49.6 ms; the longest host-side time of a warm default-stream call of a row that promises no synchronisation was 0.88 ms
(sample_images_backward), so the delay is 56 times that (at least five times is asserted, from the figures of the run itself).
The 61 tests of this file take 7.2 s there in all: about two delays per row."""
import time

import pytest

import stream_cases as sc

pytestmark = pytest.mark.gpu

DELAY_TARGET_MS, DELAY_MIN_MS = 50.0, 20.0

_state = {}


@pytest.fixture(scope="module")
def torch():
    return sc.env().torch


@pytest.fixture(scope="module")
def delay(torch):
    """delay() enqueues about DELAY_TARGET_MS of device work on the current stream; delay.ms is what one such call measured"""
    a = torch.randn(2048, 2048, device="cuda")

    def work(n):
        if hasattr(torch.cuda, "_sleep"):
            torch.cuda._sleep(int(n))
        else:
            for _ in range(int(n)):
                a.copy_(a @ a * 1e-3)

    def measure(n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        work(n)
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1)

    n = 1_000_000 if hasattr(torch.cuda, "_sleep") else 4
    measure(n)                                            # (warm)
    n = max(1, int(n * DELAY_TARGET_MS / max(measure(n), 1e-3)))
    ms = measure(n)
    print(f"delay: {n} units measured {ms:.1f} ms")
    assert ms >= DELAY_MIN_MS, f"the delay measured {ms:.1f} ms"
    assert ms <= 20 * DELAY_TARGET_MS, f"the delay measured {ms:.1f} ms: it must stay short"
    fn = lambda: work(n)
    fn.ms = ms
    fn.short = lambda: work(max(1, n // 10))
    return fn


@pytest.fixture(scope="module")
def side(torch, delay):
    """the module's side stream, one that runs BESIDE the default stream: while an event behind a tenth of the delay on it is
    still pending, an event recorded on the default stream has completed (streams that share a hardware queue fail this, see the
    module docstring).  The first of torch's streams that shows it is taken; no clock is read."""
    a = torch.zeros(1, device="cuda")
    for _ in range(8):
        stream = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            delay.short()
            behind = torch.cuda.Event()
            behind.record(stream)
        a.add_(1)                                         # (default stream)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        beside = not behind.query()
        stream.synchronize()
        if beside:
            return stream
    pytest.fail("none of eight streams runs beside the default stream: the stream checks would see nothing")


def _bits(t):
    return t.detach().contiguous().reshape(-1).view(sc.env().torch.uint8)


def _same(got, want) -> bool:
    """bit for bit, NaNs and signed zeros included"""
    torch = sc.env().torch
    if len(got) != len(want):
        return False
    for g, w in zip(got, want):
        if (g is None) != (w is None):
            return False
        if g is None:
            continue
        if g.dtype != w.dtype or g.shape != w.shape or not torch.equal(_bits(g), _bits(w)):
            return False
    return True


def _reference(row, torch):
    """the row's kept scene, its default-stream result (run twice, bit-identical) and the host time of the warm call"""
    if row.name not in _state:
        scene = row.build()
        first = scene.run(scene.real)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ref = scene.run(scene.real)
        host_ms = 1e3 * (time.perf_counter() - t0)
        torch.cuda.synchronize()
        if scene.status is not None:
            scene.status()
        assert any(t is not None and t.numel() > 0 for t in ref), "the row returns nothing to compare"
        assert _same(first, ref), "two runs on the default stream differ: the operation is not deterministic"
        _state[row.name] = (scene, ref, host_ms)
    return _state[row.name]


@pytest.mark.parametrize("row", sc.TABLE, ids=lambda r: r.name)
def test_late_inputs_on_a_side_stream(row, torch, delay, side):
    scene, ref, host_ms = _reference(row, torch)
    # the stale data is other data, and the operation notices it
    for k, t in scene.stale.items():
        assert t.shape == scene.real[k].shape and t.dtype == scene.real[k].dtype and not torch.equal(t, scene.real[k]), k
    assert not _same(scene.run(scene.stale), ref), "the stale inputs give the same result: this row could not fail"
    twins = {k: t.clone() for k, t in scene.stale.items()}
    torch.cuda.synchronize()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        delay()
        for k, t in twins.items():
            t.copy_(scene.real[k], non_blocking=True)
        filled = torch.cuda.Event()
        filled.record(side)
        t0 = time.perf_counter()
        got = scene.run(twins)                            # (an error status raises)
        returned_early = not filled.query()
        call_ms = 1e3 * (time.perf_counter() - t0)
        side.synchronize()
        if scene.status is not None:
            scene.status()
    print(f"{row.name}: host_sync={row.host_sync!r} returned_early={returned_early} call {call_ms:.2f} ms "
          f"(warm default-stream call {host_ms:.2f} ms, delay {delay.ms:.1f} ms)")
    assert _same(got, ref), "the side-stream result differs from the default-stream result: something ran off the caller's stream"
    if row.host_sync is False:
        assert returned_early, (f"documented as free of host synchronisation, but the call returned after the stream had run "
                                f"its {delay.ms:.0f} ms delay (the call took {call_ms:.1f} ms, {host_ms:.2f} ms warm on the default stream)")


def test_the_delay_covers_the_host_side_of_every_asynchronous_call(torch, delay):
    """check (b) can only tell a synchronisation from a slow call if the delay is long against the call's own host time: at least
    five times the longest warm default-stream call of a row that promises no synchronisation"""
    worst = max(((_reference(row, torch)[2], row.name) for row in sc.TABLE if row.host_sync is False))
    print(f"delay {delay.ms:.1f} ms; longest host-side call {worst[0]:.2f} ms ({worst[1]})")
    assert delay.ms >= 5.0 * worst[0], worst


@pytest.mark.parametrize("row", [r for r in sc.TABLE if r.lazy], ids=lambda r: r.name)
def test_first_use_while_the_default_stream_is_busy(row, torch, delay, side):
    _, ref, _ = _reference(row, torch)
    # a same-sized problem / handle, run and destroyed: what it leaves in the allocator's memory is not zero
    used = row.build(fresh=True)
    used.run(used.real)
    torch.cuda.synchronize()
    used.close()
    del used
    scene = row.build(fresh=True)                         # (the problem / handle exists from here on; its lazy state does not)
    torch.cuda.synchronize()
    delay()                                               # the DEFAULT stream is busy ...
    busy = torch.cuda.Event()
    busy.record()
    with torch.cuda.stream(side):
        first = scene.run(scene.real)                     # ... during the first use, on a side stream
        side.synchronize()
        was_busy = not busy.query()
        ok_first = _same(first, ref)
        torch.cuda.synchronize()
        second = scene.run(scene.real)
        side.synchronize()
    torch.cuda.synchronize()
    scene.close()
    print(f"{row.name}: the default stream was {'still busy' if was_busy else 'IDLE'} when the first use had run on the side stream")
    assert was_busy, "the first use waited for the default stream's delay: it did not run while the default stream was busy"
    assert ok_first, "the first use on a side stream differs from the default-stream result"
    assert _same(second, ref), "the second call differs: something of the first use landed after it"

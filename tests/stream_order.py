"""A harness that turns a stream-ordering mistake of one library call into a wrong answer.

include/vlg_hip.h promises that a call handed a `stream` does all its device work on that stream.  On the NULL stream everything
is ordered by accident, so the suite's other tests cannot see a launch, scan, memset or copy that was left on another stream.
StreamOrder.run makes one call on a fresh NON-BLOCKING stream S, in two passes:

  pass A, late inputs   the device inputs hold POISON and the outputs a sentinel.  On S, in this order: a delay, device-to-device copies
                        of the real inputs over the poison, the call with stream = S, a clone of every device output.  Then S is
                        synchronised and the clones are compared with the expected values.  A piece of the call that runs on another
                        stream reads the poison, or writes after the clone was taken.
  pass B, busy NULL     the real inputs are in place, the delay is enqueued on the NULL stream instead, the call and the clones go on
                        S.  A piece of the call that was left on the NULL stream runs late: what follows it on S sees unwritten data,
                        or the clone sees the sentinel.  What the call returns to the host is compared as it is returned.

THE POISON RULE.  Poison is always VALID input: in range, of the same shape and dtype as the real input, and with a correct answer that
differs from the real one in most elements (a rotated or reversed copy of the real indices, other sorted lists of the same lengths,
other ranges of the same lengths with the same output offsets).  A premature read must give a WRONG ANSWER, NEVER AN OUT-OF-BOUNDS
ACCESS.  A call with a device input for which no such poison exists runs pass B only, and its row says so.

The delay is torch.cuda._sleep, calibrated once to milliseconds with events; it is at least FLOOR_MS and at least ten times the longest
call of the table (measured on the NULL stream by the test module's fixture, which then calls set_delay).  The floor is there to dwarf
the host's cost of enqueueing a copy and a call; it is no pass criterion.  control() proves with torch alone that the harness sees a
mistake on this machine.

Not every non-blocking stream runs free of the NULL stream (the runtime spreads its streams over a few hardware queues), so new_stream()
hands out only streams on which both passes, tried in small with torch alone, do show a mistake (runs_beside_null_stream)."""
import ctypes as C

import numpy as np

FLOOR_MS = 50.0
PROBE_MS = 10.0                      # the delay of the probe that picks a stream (far above the host's cost of an event on the NULL stream)
HIP_STREAM_NON_BLOCKING = 1
SENTINEL = 0xA5                      # every byte of an output before the call


def _loaded_hip_runtime():
    """the HIP runtime this process has already loaded (torch brought it in): its path from /proc/self/maps, opened again"""
    path = None
    with open("/proc/self/maps") as f:
        for line in f:
            p = line.rsplit(" ", 1)[-1].strip()
            if "libamdhip64" in p:
                path = p
                break
    assert path, "no HIP runtime is loaded in this process"
    return C.CDLL(path)


class Case:
    """One call under test.
    inputs    [(real, poison)] device tensors of equal shape and dtype; the call reads the staging copies it is handed
    outputs   [(shape, torch dtype)] device outputs, allocated and filled with the sentinel by the harness
    call      call(stream_ptr, ins, outs, mark) -> what the call returns on the host (or None).  mark() records whether S is idle at that
              moment; a call that does more than the entry point under test (a probe behind a creation) calls it right after the entry
              point returned, otherwise the harness does when call returns
    expected  [numpy arrays] of the outputs; host: the expected return value
    verify    verify(clones as numpy, returned) for outputs that are checked otherwise than by equality
    in_place  {input number: numpy array} inputs that the call changes in place (a sort): cloned and compared like outputs
    poison_ok False: no safe poison exists for a device input -> pass B only"""

    def __init__(self, call, inputs=(), outputs=(), expected=(), host=None, verify=None, in_place=None, poison_ok=True):
        self.call, self.inputs, self.outputs, self.expected = call, list(inputs), list(outputs), list(expected)
        self.host, self.verify, self.in_place, self.poison_ok = host, verify, dict(in_place or {}), poison_ok


class StreamOrder:
    def __init__(self, torch):
        self.torch = torch
        self.hip = _loaded_hip_runtime()
        self.hip.hipStreamGetFlags.argtypes = [C.c_void_p, C.POINTER(C.c_uint)]
        self.hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        self.cycles_per_ms = self._calibrate()
        self._real = torch.arange(1 << 12, dtype=torch.int64, device="cuda")
        self._sentinel = torch.full_like(self._real, -7)
        self._tried = {}
        self.delay_ms = FLOOR_MS
        self.longest_call_ms = 0.0

    # ---- streams --------------------------------------------------------------------------------------------------------------------
    def stream_flags(self, stream):
        flags = C.c_uint(0xFFFF)
        err = self.hip.hipStreamGetFlags(C.c_void_p(stream.cuda_stream), C.byref(flags))
        assert err == 0, "hipStreamGetFlags failed: %d" % err
        return flags.value

    def _fresh_stream(self):
        """a non-blocking stream: torch's own if it is one, else one made with hipStreamNonBlocking and wrapped"""
        torch = self.torch
        s = torch.cuda.Stream()
        if not self.stream_flags(s) & HIP_STREAM_NON_BLOCKING:
            h = C.c_void_p()
            err = self.hip.hipStreamCreateWithFlags(C.byref(h), HIP_STREAM_NON_BLOCKING)
            assert err == 0 and h.value, "hipStreamCreateWithFlags failed: %d" % err
            s = torch.cuda.ExternalStream(h.value)
        assert self.stream_flags(s) & HIP_STREAM_NON_BLOCKING, "the stream under test must be non-blocking"
        return s

    def runs_beside_null_stream(self, s):
        """would a mistake show on s?  Both passes in small, with torch alone and a short delay: a write left on the NULL stream behind
        the delay must come too late for a clone on s (pass B), and a read on the NULL stream must come too early for a copy on s
        behind the delay (pass A).  The runtime spreads its streams over a few hardware queues, and on some of torch's pool streams
        (every fourth, on the machines this was written on) neither holds although the stream is non-blocking: there a piece of a call
        that was left on the NULL stream is ordered by accident, as it is on the NULL stream itself."""
        torch = self.torch
        cycles = int(PROBE_MS * self.cycles_per_ms)
        out = self._sentinel.clone()
        torch.cuda.synchronize()
        torch.cuda._sleep(cycles)                             # (the current stream is the NULL stream)
        out.copy_(self._real)
        with torch.cuda.stream(s):
            late = out.clone()
        s.synchronize()
        buf = self._sentinel.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(cycles)
            buf.copy_(self._real, non_blocking=True)
        early = buf.clone()
        torch.cuda.synchronize()
        return bool((late == self._sentinel).all()) and bool((early == self._sentinel).all())

    def new_stream(self):
        """a fresh non-blocking stream on which a mistake shows"""
        for _ in range(64):
            s = self._fresh_stream()
            if s.cuda_stream not in self._tried:              # (torch hands its pool streams out again: each is tried once)
                self._tried[s.cuda_stream] = self.runs_beside_null_stream(s)
            if self._tried[s.cuda_stream]:
                return s
        raise AssertionError("no non-blocking stream runs beside the NULL stream: the harness would be blind")

    # ---- delay ----------------------------------------------------------------------------------------------------------------------
    def _calibrate(self):
        torch = self.torch
        cycles = 1 << 20
        while True:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            torch.cuda._sleep(cycles)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
            if ms >= 5.0 or cycles >= 1 << 36:
                assert ms > 0, "torch.cuda._sleep took no time"
                return cycles / ms
            cycles *= 4

    def time_on_null_stream(self, fn):
        """milliseconds of fn() between two events on the NULL stream"""
        torch = self.torch
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def set_delay(self, longest_call_ms):
        self.longest_call_ms = float(longest_call_ms)
        self.delay_ms = max(FLOOR_MS, 10.0 * self.longest_call_ms)
        return self.delay_ms

    def delay(self, stream):
        """enqueue the delay on `stream` (None: the NULL stream)"""
        torch = self.torch
        with torch.cuda.stream(stream if stream is not None else torch.cuda.default_stream()):
            torch.cuda._sleep(int(self.delay_ms * self.cycles_per_ms))

    # ---- the control ------------------------------------------------------------------------------------------------------------------
    def control(self):
        """delay + copy-over-poison on S, a clone of the buffer issued at once on a second non-blocking stream -> (clone, poison, real):
        a harness that can see a mistake finds the clone equal to the poison"""
        torch = self.torch
        real = torch.arange(1 << 16, dtype=torch.int64, device="cuda")
        poison = torch.flip(real, [0]).contiguous()
        buf = poison.clone()
        s, other = self.new_stream(), self.new_stream()
        torch.cuda.synchronize()
        self.delay(s)
        with torch.cuda.stream(s):
            buf.copy_(real, non_blocking=True)
        with torch.cuda.stream(other):
            early = buf.clone()
        other.synchronize()
        got = early.cpu().numpy()
        torch.cuda.synchronize()
        assert np.array_equal(buf.cpu().numpy(), real.cpu().numpy())
        return got, poison.cpu().numpy(), real.cpu().numpy()

    def control_null_stream(self):
        """the same with the early clone on the NULL stream: a launch that a call leaves there runs ahead of the late inputs"""
        torch = self.torch
        real = torch.arange(1 << 16, dtype=torch.int64, device="cuda")
        poison = torch.flip(real, [0]).contiguous()
        buf = poison.clone()
        s = self.new_stream()
        torch.cuda.synchronize()
        self.delay(s)
        with torch.cuda.stream(s):
            buf.copy_(real, non_blocking=True)
        early = buf.clone()                                   # (the current stream is the NULL stream)
        ev = torch.cuda.Event()
        ev.record()
        ev.synchronize()
        got = early.cpu().numpy()
        torch.cuda.synchronize()
        return got, poison.cpu().numpy(), real.cpu().numpy()

    # ---- one call, one pass ---------------------------------------------------------------------------------------------------------
    def run(self, case, which):
        """which: "A" or "B" -> whether S was idle when the entry point returned"""
        torch = self.torch
        assert which in ("A", "B")
        s = self.new_stream()
        ins = [(poison if which == "A" else real).clone() for real, poison in case.inputs]
        outs = []
        for shape, dtype in case.outputs:
            o = torch.empty(shape, dtype=torch.uint8, device="cuda") if dtype is None else torch.empty(shape, dtype=dtype, device="cuda")
            o.view(torch.uint8).fill_(SENTINEL)
            outs.append(o)
        idle = []
        torch.cuda.synchronize()
        self.delay(s if which == "A" else None)
        with torch.cuda.stream(s):
            if which == "A":
                for buf, (real, _) in zip(ins, case.inputs):
                    buf.copy_(real, non_blocking=True)
            returned = case.call(s.cuda_stream, ins, outs, lambda: idle.append(s.query()))
            if not idle:
                idle.append(s.query())
            clones = [o.clone() for o in outs] + [ins[j].clone() for j in sorted(case.in_place)]
        s.synchronize()
        got = [c.cpu().numpy() for c in clones]
        torch.cuda.synchronize()                              # (the delay of pass B, before the next test)
        if case.verify is not None:
            case.verify(got, returned)
        for j, (g, want) in enumerate(zip(got, case.expected + [case.in_place[j] for j in sorted(case.in_place)])):
            want = np.asarray(want)
            g = g.view(want.dtype) if g.dtype != want.dtype and g.dtype.itemsize == want.dtype.itemsize else g
            bad = np.flatnonzero(g.reshape(-1) != want.reshape(-1))
            assert not len(bad), "pass %s: output %d differs in %d of %d elements, first at %d: got %r, expected %r" % (
                which, j, len(bad), want.size, int(bad[0]), g.reshape(-1)[bad[0]], want.reshape(-1)[bad[0]])
        if case.host is not None:
            assert len(returned) == len(case.host)
            for j, (g, want) in enumerate(zip(returned, case.host)):
                assert np.array_equal(np.asarray(g), np.asarray(want)), "pass %s: returned value %d differs" % (which, j)
        return idle[0]

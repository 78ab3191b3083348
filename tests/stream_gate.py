"""A gate that makes stream ordering observable (helper of tests/test_gpu_streams.py; no library code).

On a torch stream `s`, with no host wait in between and every tensor allocated under `with torch.cuda.stream(s)`:
  1. a delay (torch.cuda._sleep; a chain of float64 matmuls where _sleep does not delay),
  2. a copy_ of every real operand into a tensor prefilled with NaN,
  3. the library calls under test, on the tensors' data_ptr(),
  4. a copy of every tensor the calls may have written into a tensor prefilled with SENTINEL,
and only then s.synchronize().  A piece of a call that ran on another stream, or ahead of the stream's order, reads NaN;
a piece that ran behind the stream's order leaves the output's NaN prefill (or, had the copy itself not run, SENTINEL)
in the copy.

Gate and Plain offer the same methods, so that one function runs a case behind the gate on the handle under test and
with host waits on the reference handle (a second handle of the same problem on its own stream).

The delay: GATE_MS, forty times ENQUEUE_MS -- the longest the host took to enqueue a call under test on an idle handle
(profiles/caller_stream.md has both measurements) -- and below 100 ms.  _sleep counts clock cycles, so its rate is measured
once per process; every gate then measures its own delay with events on `s` (Gate.delays).  One gate in about a thousand
was measured at a third of what it asked for (9.5 ms, still nine times the enqueue time), so a single gate is refused
only below MIN_GATE_MS, where the delay has stopped delaying; the timer test compares with the measured value."""
import numpy as np

GATE_MS = 40.0       # what a gate asks for
ENQUEUE_MS = 1.0     # upper bound of the measured enqueue time of the slowest call, 0.97 ms (profiles/caller_stream.md)
MIN_GATE_MS = 3.0 * ENQUEUE_MS
SENTINEL = -7.25
_RATE = {}           # "sleep": cycles per ms | "matmul": products per ms


def _torch():
    import torch
    return torch


def _timed(fn):
    torch = _torch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _matmul_chain(n):
    torch = _torch()
    a = _RATE.setdefault("matrix", torch.full((512, 512), 1.0 / 512, dtype=torch.float64, device="cuda:0"))
    b = a
    for _ in range(int(n)):
        b = a @ b
    return b


def calibrate():
    """Measures once how fast the delay runs (on the current stream, with host waits)."""
    if "kind" in _RATE:
        return _RATE
    torch = _torch()
    torch.cuda._sleep(1000)
    torch.cuda.synchronize()
    cycles = 4_000_000
    ms = min(_timed(lambda: torch.cuda._sleep(cycles)) for _ in range(2))
    if 0.2 <= ms <= 400.0:
        _RATE.update(kind="sleep", per_ms=cycles / ms)
    else:  # _sleep does not delay here: a chain of matmuls
        _matmul_chain(8)
        torch.cuda.synchronize()
        ms = min(_timed(lambda: _matmul_chain(400)) for _ in range(2))
        _RATE.update(kind="matmul", per_ms=400 / ms)
    return _RATE


def delay(ms):
    """Enqueues about `ms` milliseconds of work on the current torch stream."""
    r = calibrate()
    n = max(1, int(r["per_ms"] * ms))
    if r["kind"] == "sleep":
        _torch().cuda._sleep(n)
    else:
        _matmul_chain(n)


_STREAMS = {}
KINDS = ("plain", "high", "zero")


def stream(kind):
    """The three kinds of caller's stream, one of each per process (a handle may stay on one after a test)."""
    torch = _torch()
    if kind not in _STREAMS:
        _STREAMS[kind] = {"plain": lambda: torch.cuda.Stream(), "high": lambda: torch.cuda.Stream(priority=-1),
                          "zero": lambda: torch.cuda.default_stream(), "second": lambda: torch.cuda.Stream()}[kind]()
    return _STREAMS[kind]


def stream_ptr(s):
    return int(s.cuda_stream)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.uint64)


def same(a, b):
    """Bit-for-bit equality of nested results (dicts, sequences, arrays, numbers)."""
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape:
        return False
    if a.dtype.kind == "f" or b.dtype.kind == "f":
        return bool(np.array_equal(bits(a), bits(b)))
    return bool(np.array_equal(a, b))


def differing(a, b, path=""):
    """Names of the entries of two nested results that are not the same bits."""
    if isinstance(a, dict) and isinstance(b, dict) and a.keys() == b.keys():
        return [n for k in a for n in differing(a[k], b[k], "%s/%s" % (path, k))]
    return [] if same(a, b) else [path or "/"]


class Buf:
    """A device buffer of a case: .ptr for the library, .tensor where torch owns it."""

    def __init__(self, ptr, k, tensor=None, doubles=None):
        self.ptr, self.k, self.tensor, self.doubles = ptr, k, tensor, doubles


class Gate:
    """Operands and results of library calls on handle `ctx`, which is on the torch stream `s`, behind a delay."""

    def __init__(self, ctx, s, ms=GATE_MS, min_ms=MIN_GATE_MS):
        torch = _torch()
        calibrate()
        self.ctx, self.s, self.ms, self.min_ms = ctx, s, ms, min_ms
        self.rows = int(ctx.rows)
        self.staged, self.watched, self.snaps, self.events = [], [], {}, []
        self.open_count = 0
        self._cm = None
        self.torch = torch

    # ---- buffers (all before the gate opens)
    def _new(self, n, fill):
        with self.torch.cuda.stream(self.s):
            return self.torch.full((max(int(n), 1),), fill, dtype=self.torch.float64, device="cuda:0")

    def operand(self, host, k=None):
        """A resident vector holding the N x k host matrix, readable only once the gate has opened."""
        host = np.asarray(host, dtype=np.float64)
        host = host.reshape(len(host), -1)
        k = host.shape[1] if k is None else k
        n = self.rows * max(k, 2)
        real, target = self._new(n, 0.0), self._new(n, float("nan"))
        v = self.ctx.dev_alloc(k)
        self.ctx.upload(host, v)
        self.ctx.copy_dev(v, k, real.data_ptr())
        self.ctx.sync()
        self.ctx.dev_free(v)
        self.staged.append((target, real))
        b = Buf(target.data_ptr(), k, target)
        self.watched.append(b)
        return b

    def result(self, k):
        """A resident vector of k columns prefilled with NaN."""
        t = self._new(self.rows * max(k, 2), float("nan"))
        b = Buf(t.data_ptr(), k, t)
        self.watched.append(b)
        return b

    def raw_operand(self, values):
        """Plain device doubles (thresholds, weights), readable only once the gate has opened."""
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        with self.torch.cuda.stream(self.s):
            real = self.torch.from_numpy(np.concatenate([values, np.zeros(1)])).to("cuda:0")
        self.s.synchronize()
        target = self._new(len(values) + 1, float("nan"))
        self.staged.append((target, real))
        b = Buf(target.data_ptr(), None, target, len(values))
        self.watched.append(b)
        return b

    def raw_result(self, n):
        t = self._new(n + 1, float("nan"))
        b = Buf(t.data_ptr(), None, t, int(n))
        self.watched.append(b)
        return b

    # ---- the gate
    def open(self, stage=True):
        """Enqueues the delay (and, the first time, the copies of the real operands) on s; no host wait."""
        torch = self.torch
        with torch.cuda.stream(self.s):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            delay(self.ms)
            e1.record()
            self.events.append((e0, e1))
            if stage and self.open_count == 0:
                for target, real in self.staged:
                    target.copy_(real)
        self.open_count += 1

    def between(self, buf):
        """A torch kernel on s that reads and rewrites `buf` (the same values): work of the caller between two calls."""
        with self.torch.cuda.stream(self.s):
            buf.tensor.copy_(buf.tensor.clone())

    def snapshot(self):
        """Enqueues the copy of every buffer into a SENTINEL tensor on s; no host wait."""
        with self.torch.cuda.stream(self.s):
            for b in self.watched:
                snap = self.torch.full_like(b.tensor, SENTINEL)
                snap.copy_(b.tensor)
                self.snaps[id(b)] = snap

    def wait(self):
        self.s.synchronize()
        self.delays = [e0.elapsed_time(e1) for e0, e1 in self.events]
        assert all(ms >= self.min_ms for ms in self.delays), "a gate of %s ms is too short to order anything" % self.delays
        for b in self.watched:
            assert not bool((self.snaps[id(b)] == SENTINEL).any().item()), "the copy after the calls did not run"

    def __enter__(self):
        self.open()
        self._cm = self.torch.cuda.stream(self.s)
        self._cm.__enter__()
        return self

    def __exit__(self, *exc):
        self._cm.__exit__(*exc)
        if exc[0] is None:
            self.snapshot()
            self.wait()
        else:
            self.s.synchronize()
        return False

    # ---- results (after wait)
    def host(self, b):
        """The N x k matrix a resident buffer held when the calls had run."""
        return self.ctx.download(self.snaps[id(b)].data_ptr(), b.k)

    def raw(self, b):
        return self.snaps[id(b)].cpu().numpy()[:b.doubles]

    def free(self):
        pass


class Plain:
    """The same buffers on a handle that stays on its own stream, with host waits: the reference."""

    def __init__(self, ctx):
        self.ctx, self.torch = ctx, _torch()
        self.vecs = []

    def operand(self, host, k=None):
        host = np.asarray(host, dtype=np.float64)
        host = host.reshape(len(host), -1)
        k = host.shape[1] if k is None else k
        v = self.ctx.dev_alloc(k)
        self.ctx.upload(host, v)
        self.vecs.append(v)
        return Buf(v, k)

    def result(self, k):
        v = self.ctx.dev_alloc(k)
        self.ctx.upload(np.full((self.ctx.N, k), np.nan), v)   # prefilled like the gate's
        self.vecs.append(v)
        return Buf(v, k)

    def raw_operand(self, values):
        values = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        t = self.torch.from_numpy(np.concatenate([values, np.zeros(1)])).to("cuda:0")
        self.torch.cuda.synchronize()
        return Buf(t.data_ptr(), None, t, len(values))

    def raw_result(self, n):
        t = self.torch.full((n + 1,), float("nan"), dtype=self.torch.float64, device="cuda:0")
        self.torch.cuda.synchronize()
        return Buf(t.data_ptr(), None, t, int(n))

    def open(self, stage=True):
        self.ctx.sync()

    def between(self, buf):
        self.ctx.sync()
        buf.tensor.copy_(buf.tensor.clone())
        self.torch.cuda.synchronize()

    def snapshot(self):
        pass

    def wait(self):
        self.ctx.sync()
        self.torch.cuda.synchronize()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.wait()
        return False

    def host(self, b):
        return self.ctx.download(b.ptr, b.k)

    def raw(self, b):
        self.ctx.sync()
        return b.tensor.cpu().numpy()[:b.doubles]

    def free(self):
        for v in self.vecs:
            self.ctx.dev_free(v)
        self.vecs = []

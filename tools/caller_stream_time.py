"""What tests/stream_gate.py's constants rest on (profiles/caller_stream.md): the rate of the gate's delay, the measured
length of a gate, and how long the host takes to enqueue each call under test on an idle handle -- host clock around the
call and torch events on the handle's stream, best of three.  python tools/caller_stream_time.py"""
import json
import os
import sys
import time


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import stream_gate as sg  # noqa: E402
import test_gpu_streams as T  # noqa: E402

out = {}
rate = sg.calibrate()
out["delay"] = {k: v for k, v in rate.items() if k in ("kind", "per_ms")}
s = sg.stream("plain")
with torch.cuda.stream(s):
    ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sg.delay(sg.GATE_MS)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
out["gate_ms_measured"] = ms

calls = {}


def timed(name, c, fn):
    best = None
    for _ in range(3):
        c.sync()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record(s)
        s.synchronize()
        v = (1e3 * (t1 - t0), e0.elapsed_time(e1))
        best = v if best is None or v[0] < best[0] else best
    calls[name] = dict(host_ms=best[0], events_ms=best[1])


for precond, pname in ((T.JACOBI, "jacobi"), (T.CHOLESKY, "cholesky")):
    for d, p in ((3, 5), (3, 24)):
        t, r, D = T.pair(d, p, precond)
        T.on(t, "plain")
        c = t.h
        c.set_point(D["Y"])
        B = sg.Plain(c)
        tag = "%s d%dp%d " % (pname, d, p)
        y, v, x10 = B.operand(D["Y"]), B.operand(D["V"]), B.operand(D["X"][:, :10])
        o, o10 = B.result(p), B.result(10)
        w = [B.result(p) for _ in range(5)]
        if precond == T.JACOBI:
            timed(tag + "spmm k=10", c, lambda: c.spmm_dev(x10.ptr, 10, o10.ptr))
            timed(tag + "set_point+hvp", c, lambda: (c.set_point_dev(y.ptr), c.hvp_dev(v.ptr, o.ptr)))
            timed(tag + "certificate k=10", c, lambda: c.certificate_product_dev(x10.ptr, 10, o10.ptr))
            calls_, _ = T.rowops_calls(c, B, D)
            timed(tag + "row operations (8 calls)", c, lambda: [f() for f in calls_])
            timed(tag + "dots", c, lambda: c.dots_dev([(y.ptr, v.ptr), (v.ptr, v.ptr)]))
            timed(tag + "gram", c, lambda: c.gram_dev(x10.ptr, 10, v.ptr, p))
            timed(tag + "objective", c, lambda: c.objective_dev(y.ptr))
        timed(tag + "precondition", c, lambda: c.precondition_projected_dev(v.ptr, o.ptr))
        G = c.download(c.point_ptrs()[2], p)
        g = B.operand(G)
        timed(tag + "stpcg 8 iterations", c, lambda: c.stpcg_dev(g.ptr, 1e30, *[b.ptr for b in w], kappa_fgr=1e-300, theta=0.0,
                                                                  max_iters=8))
        sv = B.operand(D["S"])
        timed(tag + "trial+accept", c, lambda: (c.set_point_dev(y.ptr), c.tnt_trial_dev(sv.ptr, w[0].ptr, w[1].ptr),
                                                c.tnt_accept_dev(w[1].ptr, w[2].ptr)))
        B.free()
out["calls"] = calls
out["slowest"] = max(calls.items(), key=lambda kv: kv[1]["host_ms"])
print(json.dumps(out["delay"]), out["gate_ms_measured"])
for k, v in calls.items():
    print("%-45s host %.3f ms  events %.3f ms" % (k, v["host_ms"], v["events_ms"]))
print("slowest", out["slowest"])

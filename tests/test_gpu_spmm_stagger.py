"""The staggered start of k_spmm's pose slices (SpmmArgs::stagger_ticks, profiles/hvp_stagger.md): a pose slice that is
the second wavefront on its SIMD sleeps before its first load.  A wavefront's arithmetic does not depend on when it starts,
so every product must keep its bits whatever the delay; the delay-0 products are checked against the oracle as
tests/test_gpu_parity.py does (1e-10 relative to the largest entry).

Small problems take neither the window form nor the gate by themselves, and their few wavefronts are alone on their
SIMDs: the tests force the window form with cora_debug_spmm_window_min_slices(0) and the gate with
cora_debug_spmm_stagger_force -- 2: every pose slice waits (the 2-pose last slice of the 130-pose chain among them),
1: the rule as large launches run it."""
import numpy as np
import pytest
import torch

from cora_amd import capi
from oracle import oracle as orc
from synth import make_problem

REL = 1e-10
DELAYS = ((50, 2), (2000, 2), (50, 1))  # (ticks of 10 ns, force): a short wait, the clamp (20 us), the residency rule
GRAPHS = {
    # 4 chain slices, 5 range slices, landmark rows of several pieces
    "ranges": dict(d=3, n=200, n_landmarks=2, n_ranges=300),
    # 3 chain slices, the last of 2 poses
    "chain130": dict(d=3, n=130, n_landmarks=0, n_ranges=0),
}


def relerr(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def same_bits(a, b):
    return torch.equal(torch.from_numpy(np.ascontiguousarray(a)), torch.from_numpy(np.ascontiguousarray(b)))


@pytest.fixture
def gate():
    """Window form and gate forced on for the duration of a test; yields the library (the delay is the test's to set)."""
    L = capi.load()
    win = L.cora_debug_spmm_window_min_slices(0)
    force = L.cora_debug_spmm_stagger_force(2)
    ticks = L.cora_debug_spmm_stagger_ticks(-1)
    yield L
    L.cora_debug_spmm_stagger_ticks(ticks)
    L.cora_debug_spmm_stagger_force(force)
    L.cora_debug_spmm_window_min_slices(win)


_problems = {}


def problem(name):
    if name not in _problems:
        _problems[name] = make_problem(seed=9, **GRAPHS[name])
    return _problems[name]


@pytest.mark.gpu
@pytest.mark.parametrize("p", [3, 5, 8])
@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_products_keep_their_bits_under_every_delay(graph, p, gate):
    A, Q, dm = problem(graph)
    rng = np.random.default_rng(p)
    Y = orc.project_manifold(dm, rng.uniform(-1, 1, (dm.N, p)))
    G = orc.egrad(Q, Y)
    V = orc.tangent_proj(dm, Y, rng.uniform(-1, 1, (dm.N, p)))
    X = rng.standard_normal((dm.N, p))
    st, ob = orc.lambda_blocks(Q, dm, Y)
    c = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val)
    c.set_rank(p)

    def products():
        # (the Hvp with a gradient from outside leaves ITS Lambda on the handle: every round starts from the point again,
        # so that the certificate product sees the same Lambda each time)
        c.set_point(Y)
        return (c.dataMatrixProduct(X), c.certificate_product(X), c.Riemannian_Hessian_vector_product(Y, G, V))

    gate.cora_debug_spmm_stagger_ticks(0)
    base = products()
    for got, ref in zip(base, (orc.spmm(Q, X), orc.S_apply(Q, dm, st, ob, X), orc.hvp(Q, dm, Y, G, V))):
        assert relerr(got, ref) < REL
    for delay, force in DELAYS:
        gate.cora_debug_spmm_stagger_ticks(delay)
        gate.cora_debug_spmm_stagger_force(force)
        for name, got, ref in zip(("Q X", "(Q - Lambda) X", "Hvp"), products(), base):
            assert same_bits(got, ref), "%s differs with a delay of %d ticks (force %d)" % (name, delay, force)
    c.close()


@pytest.mark.gpu
def test_stpcg_is_bit_equal_with_the_gate_on(gate):
    """Up to five iterations of the device STPCG (the product with the kappa slots, EPI_HVP_K): the slots are per block
    and added in block order, so the iteration count, the step's norm and every vector keep their bits."""
    A, Q, dm = problem("ranges")
    p = 5
    rng = np.random.default_rng(3)
    Y = orc.project_manifold(dm, rng.uniform(-1, 1, (dm.N, p)))
    g0 = orc.tangent_proj(dm, Y, orc.egrad(Q, Y))
    runs = []
    for delay in (0, 50, 2000):
        gate.cora_debug_spmm_stagger_ticks(delay)
        c = capi.Context(dm.d, dm.n, dm.r, dm.n_trans, Q.rowptr, Q.col, Q.val)
        c.set_rank(p)
        y, g, s, r, v, pk, hp = (c.dev_alloc(p) for _ in range(7))
        c.upload(Y, y)
        c.set_point_dev(y)
        c.upload(g0, g)
        c.precond_setup(capi.PRECOND_NONE)
        iters, step_norm = c.stpcg_dev(g, 1e6, s, r, v, pk, hp, max_iters=5)
        runs.append((iters, step_norm, [c.download(q, p) for q in (s, r, pk, hp)]))
        c.close()
    # (at most five iterations; at this random point the Hessian is indefinite and the solve may end on negative
    # curvature before the fifth -- every iteration it does run starts with one product with the kappa slots)
    assert 1 <= runs[0][0] <= 5
    for iters, step_norm, vecs in runs[1:]:
        assert iters == runs[0][0] and step_norm == runs[0][1]
        for got, ref in zip(vecs, runs[0][2]):
            assert same_bits(got, ref)


def test_delay_is_stored_clamped():
    """Host side only: the setter clamps to 0 .. 2 000 ticks, a negative argument queries."""
    L = capi.load()
    old = L.cora_debug_spmm_stagger_ticks(-1)
    try:
        L.cora_debug_spmm_stagger_ticks(1 << 20)
        assert L.cora_debug_spmm_stagger_ticks(-1) == 2000
        L.cora_debug_spmm_stagger_ticks(2001)
        assert L.cora_debug_spmm_stagger_ticks(-1) == 2000
        assert L.cora_debug_spmm_stagger_ticks(137) == 2000 and L.cora_debug_spmm_stagger_ticks(-1) == 137
        assert L.cora_debug_spmm_stagger_ticks(0) == 137 and L.cora_debug_spmm_stagger_ticks(-1) == 0
        force = L.cora_debug_spmm_stagger_force(-1)
        assert L.cora_debug_spmm_stagger_force(7) == force and L.cora_debug_spmm_stagger_force(force) == 2
    finally:
        L.cora_debug_spmm_stagger_ticks(old)

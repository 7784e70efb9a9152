"""
The Lambda half of the dmk_rccsd handle ("Lambda") through the C ABI alone, as tests/test_gpu_ccsd_shapes.py does for
the T half: dmk_rccsd_lambda_{init,set,update,run}, dmk_rccsd_rdm1, dmk_rccsd_residual, dmk_rccsd_lagrangian.  No device SCF and no
dmk_ao2mo_s4: the Fock matrix and the seven blocks come from ccsd_ref.restricted_blocks at HOST orbitals, the packed (vv|vv) block
with a pitch of npair + 3 whose pad is NaN, so only csrc/ccsd.hip is under test and a handle that dropped the pitch in the adjoint
ladder, or read the pad, gives NaN.

Uneven shapes   (o, v) with extents of 1, o o at and just above the 64-row tile of the products ((8, 9): 64, (9, 2): 81), o v and v v
                above 64 with the other side small, one side beyond the 32-tile of the permute; every case as it stands and with
                occupied-virtual rotated orbitals; random symmetric t and l of scale 0.1.  ONE sweep (lambda_set + lambda_update)
                against cclambda_ref.lambda_step_reverse element by element, the density against cclambda_ref.rdm1_reverse (both
                reverse-mode derivatives of the spin-orbital AMPLITUDE equations: no Lambda equation and no density formula on the
                reference side), the residual against r_residual with nothing divided, the Lagrangian against lagrangian: TOL = 1e-10,
                the project's one-step bound (the T suite measures 1e-16, so a real defect is orders above it).  gamma = gamma^T in
                every bit, every output finite, a second lambda_set + lambda_update gives the same bits.
Run loop        (2, 3), coupling 2.0 (cclambda_ref.coupled_system), T converged on the handle first (tol_e = 1e-12, tol_normt =
                1e-10), Lambda at 1e-10, the reference cclambda_ref.lambda_by_jacobian at the DEVICE's own t.  A ring of one vector is
                plain sweeping bit for bit, and the plain run lands within 1e-8 = 100 x the tolerance of the reference (the last step
                bounds the error only up to 1 / (1 - rho): tests/test_gpu_cclambda.py).  Rings of 2, 3 and 12 converge, take more
                sweeps than they have slots and land within the same bound -- FROM cclambda_ref.run_loop_start, a random l of scale
                0.1: from l = t this system is 2.5e-4 from its solution and a ring of 12 converges in 9 sweeps, before it is full (the
                21 plain sweeps that tests/test_host_cclambda.py pins say nothing about the count with DIIS).  That host file runs the
                same iteration over the reference sweep (cclambda_ref.lambda_run_ref) and pins both facts: 9 sweeps from l = t, and
                more sweeps than slots from the random start for every ring used here.  The runs from l = t are kept as well
                (convergence and the bound).  max_iter = 0 returns (0, 0, 0) and leaves l alone (l = t where there was none);
                max_iter = 1 without a ring is one lambda_update bit for bit and reports the 2-norm of its step; an unconverged exit
                from a ring of 4 is a state a later run converges from; solver/cc_lambda.py with diis_space = 0 against its ring of 8.
Stale state     bit for bit at (2, 3) and (8, 9): after t changed on a handle that already made a sweep (through dmk_rccsd_set, _update,
                _init, _run) the next sweep is the one of a fresh handle that only ever saw the new t; dmk_rccsd_energy, _residual,
                _lagrangian and _rdm1 between two sweeps (they overwrite the buffers the sweep uses as adjoints) change neither the
                sweep nor their own results.
Memory          residual and lagrangian need no Lambda allocation; the first lambda_set makes it, the second does not; dmk_rccsd_free
                gives everything back.
Refusals        DMK_ERR_STATE before t / before l, DMK_ERR_INVALID for NULL pointers, max_iter < 0 and a NULL result.

Measured        uneven shapes: sweep at most 5.9e-16 (l1 at (33, 3)), density 2.7e-15 ((8, 9) rotated), residual 4.4e-16, Lagrangian
                1.8e-15 ((33, 3), |L| = 4.6); no case takes more than 1.7 s.  Run loop: plain and ring of 1 take 21 sweeps and end
                2.7e-11 from the reference (max|l - t| = 2.5e-4); from the random start rings of 2, 3, 12 take 18, 14, 16 sweeps (the
                reference iteration on the host: the same three counts) and end within 1.3e-11; from l = t 12, 10, 9 sweeps, within
                6.7e-12.  One plain iteration reports |dl| = 0.72005273955179172, the host norm to the last bit.  Ring of 4: |dl| =
                2.0e-5 after 3 sweeps, converged after 7 more, 6.5e-12 from the reference.  RCCSDLambda without a ring: 38 T
                iterations and 21 sweeps (ring of 8: 13 and 9), 2.3e-11 between the two l.  Memory at o = v = 24, ring of 2: the first
                lambda_set takes 37748736 bytes (plan 37287936), everything else 0, after free 0 below the start.
                Sensitivity (shown once on scratch builds): the 0.5 of the Lovov / Wvoovb line of lambda_update changed to 0.25 fails
                all 18 uneven-shape cases and the five run-loop tests that compare with the reference; dmk_rccsd_set without its
                kept = false fails the two "set" cases of the stale-state test and nothing else.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import ccsd_ref as CR
from tests import cclambda_ref as LR
from tests.test_gpu_ccsd_shapes import DMK_OK, DMK_ERR_INVALID, DMK_ERR_STATE, L1, L2, PAD, TOL, Handle, _bits, _host

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (1, 2), (5, 1), (1, 33), (9, 2), (8, 9), (33, 3), (3, 33)]
RUN_SHAPE, RUN_SCALE = (2, 3), 2.0
TOL_L = 1e-10                      # |dl|_2 of the run-loop tests
NEAR = 100.0 * TOL_L               # converged l against the Jacobian reference
STALE = [(2, 3), (8, 9)]


@pytest.fixture(scope="module")
def ctx():
    from libdmet_preview_amd import _lib
    return _lib.get_ctx()


def _same(a, b):
    return all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _far(a, b):
    return max(np.abs(x - y).max() for x, y in zip(a, b))


# ---- uneven shapes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rotated", [False, True])
@pytest.mark.parametrize("o,v", SHAPES)
def test_sweep_density_residual_and_lagrangian_at_uneven_shapes(ctx, o, v, rotated):
    so, fock, blocks = _host(o, v, rotated)
    n = o + v
    assert np.all(np.isnan(blocks["vvvv"][:, -PAD:]))
    rng = np.random.default_rng(300 + 7 * o + v)
    t1, t2 = CR.random_amplitudes(rng, o, v)
    l1, l2 = CR.random_amplitudes(rng, o, v)
    n_ref = LR.lambda_step_reverse(so, t1, t2, l1, l2)
    g_ref = LR.rdm1_reverse(so, t1, t2, l1, l2)
    r_ref = LR.r_residual(so, t1, t2)
    L_ref = float(LR.lagrangian(so, t1, t2, l1, l2))
    h = Handle(ctx, o, v, fock, blocks, diis=0)
    try:
        h.set(t1, t2)
        h.lambda_set(l1, l2)
        h.lambda_update()
        n_dev = h.lams()
        h.lambda_set(l1, l2)
        gam = h.rdm1()
        r_dev = h.residual()
        L_dev = h.lagrangian(l1, l2)
        h.lambda_update()
        m_dev = h.lams()
    finally:
        h.close()
    errs = (np.abs(n_dev[0] - n_ref[0]).max(), np.abs(n_dev[1] - n_ref[1]).max(), np.abs(gam - g_ref).max(),
            np.abs(r_dev[0] - r_ref[0]).max(), np.abs(r_dev[1] - r_ref[1]).max(), abs(L_dev - L_ref))
    print("(o, v) = (%d, %d)%s: sweep max|d l1| = %.3e max|d l2| = %.3e;  density %.3e;  residual max|d r1| = %.3e max|d r2| = %.3e;  "
          "|d L| = %.3e  (max|l2new| = %.3f, max|r2| = %.3f, L = %.6f)"
          % ((o, v, " rotated" if rotated else "") + errs + (np.abs(n_ref[1]).max(), np.abs(r_ref[1]).max(), L_ref)))
    for x in n_dev + (gam,) + r_dev + (L_dev,):
        assert np.all(np.isfinite(x))
    assert n_dev[0].shape == (o, v) and n_dev[1].shape == (o, o, v, v) and gam.shape == (n, n)
    assert max(errs) <= TOL
    assert np.array_equal(_bits(gam), _bits(gam.T))
    assert _same(n_dev, m_dev)                                       # two sweeps, the same bits (the second on kept intermediates)


# ---- the run loop --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _run_case():
    """(spin-orbital Hamiltonian, Fock matrix, blocks) of the (2, 3) system at coupling 2.0, host orbitals: shared, never modified."""
    o, v = RUN_SHAPE
    sysm, Cmo = LR.coupled_system(o, v, RUN_SCALE)
    return (CR.spin_orbital(sysm, Cmo, o),) + CR.restricted_blocks(sysm, Cmo, o, pad=PAD)


_REFERENCE = {}


def _reference(t1, t2):
    """lambda_by_jacobian at the amplitudes given (one solve per distinct t)."""
    key = t1.tobytes() + t2.tobytes()
    if key not in _REFERENCE:
        _REFERENCE[key] = LR.solve_lambda_ref(_run_case()[0], t1, t2)
    return _REFERENCE[key]


def _run_handle(ctx, diis):
    """A handle of the run-loop system with T converged on it."""
    _, fock, blocks = _run_case()
    h = Handle(ctx, RUN_SHAPE[0], RUN_SHAPE[1], fock, blocks, diis=diis)
    try:
        assert h.run(200)[1] == 1.0
    except BaseException:
        h.close()
        raise
    return h


def _solve(ctx, diis, max_iter=200, start=None):
    """T, then Lambda from `start` (default: from l = t): (result of lambda_run, (t1, t2), (l1, l2), max|l - l_ref|)."""
    h = _run_handle(ctx, diis)
    try:
        if start is not None:
            h.lambda_set(*start)
        res = h.lambda_run(max_iter, TOL_L)
        t, l = h.amps(), h.lams()
    finally:
        h.close()
    return res, t, l, _far(l, _reference(*t))


def test_a_ring_of_one_vector_is_plain_sweeping_bit_for_bit(ctx):
    (r0, t0, l0, err0), (r1, t1, l1, err1) = _solve(ctx, 0), _solve(ctx, 1)
    print("ring 0: %d sweeps, |dl| = %.3e, max|l - l_ref| = %.3e;  ring 1: %d sweeps, max|l - l_ref| = %.3e;  max|l - t| = %.3e"
          % (r0[1], r0[2], err0, r1[1], err1, _far(l0, t0)))
    assert r0[0] == 1.0 and r1[0] == 1.0 and r0[1] == r1[1] and r0[1] > 12          # (the host reference: 21 plain sweeps)
    assert _same(t0, t1) and _same(l0, l1) and np.array_equal(_bits(r0[2]), _bits(r1[2]))
    assert 0.0 < r0[2] < TOL_L and err0 <= NEAR                                    # the plain run lands on the reference
    assert _far(l0, t0) > 1e-5                                                      # and l is not t


@pytest.mark.parametrize("diis", [2, 3, 12])
def test_rings_wrap_and_converge_to_the_reference(ctx, diis):
    """From cclambda_ref.run_loop_start, a random l of scale 0.1: from l = t this system is 2.5e-4 from its solution and a ring of 12
    converges in 9 sweeps, before it is full (the device and the reference iteration of tests/test_host_cclambda.py agree on that
    count); from the random start the reference iteration takes 18, 14 and 16 sweeps with rings of 2, 3 and 12."""
    res, t, l, err = _solve(ctx, diis, start=LR.run_loop_start(*RUN_SHAPE))
    near, t_near, l_near, err_near = _solve(ctx, diis)               # and from l = t, where only the small rings wrap
    print("ring %d: converged %d after %d sweeps, |dl| = %.3e, max|l - l_ref| = %.3e;  from l = t: converged %d after %d sweeps, %.3e"
          % (diis, res[0], res[1], res[2], err, near[0], near[1], err_near))
    assert res[0] == 1.0 and res[1] > diis                           # more sweeps than slots: the ring wrapped
    assert res[2] < TOL_L and err <= NEAR
    assert near[0] == 1.0 and near[2] < TOL_L and err_near <= NEAR and _far(l, l_near) <= 2.0 * NEAR
    assert np.abs(l[1] - l[1].transpose(1, 0, 3, 2)).max() <= 1e-12


@pytest.mark.parametrize("diis", [0, 4])
def test_no_sweeps_leave_lambda_alone(ctx, diis):
    o, v = RUN_SHAPE
    l_in = CR.random_amplitudes(np.random.default_rng(21), o, v)
    h = _run_handle(ctx, diis)
    try:
        res_none = h.lambda_run(0, TOL_L)                            # no l yet: l = t
        t, l_none = h.amps(), h.lams()
        h.lambda_set(*l_in)
        res_set = h.lambda_run(0, TOL_L)
        l_set = h.lams()
    finally:
        h.close()
    assert res_none == (0.0, 0.0, 0.0) and res_set == (0.0, 0.0, 0.0)
    assert _same(l_none, t) and _same(l_set, l_in)


def test_one_plain_iteration_is_one_update(ctx):
    o, v = RUN_SHAPE
    l_in = CR.random_amplitudes(np.random.default_rng(22), o, v)
    h = _run_handle(ctx, 0)
    try:
        h.lambda_set(*l_in)
        res = h.lambda_run(1, TOL_L)
        a = h.lams()
        h.lambda_set(*l_in)
        h.lambda_update()
        b = h.lams()
    finally:
        h.close()
    step = np.sqrt(np.sum((b[0] - l_in[0]) ** 2) + np.sum((b[1] - l_in[1]) ** 2))
    print("one plain iteration: |dl| reported %.17e, host 2-norm of the step %.17e (relative difference %.3e)"
          % (res[2], step, abs(res[2] - step) / step))
    assert res[:2] == (0.0, 1.0) and _same(a, b)
    assert step > 1e-3 and abs(res[2] - step) <= 1e-14 * step


def test_an_unconverged_exit_is_a_state_to_go_on_from(ctx):
    h = _run_handle(ctx, 4)
    try:
        res = h.lambda_run(3, TOL_L)
        mid = h.lams()
        again = h.lambda_run(200, TOL_L)
        t, l = h.amps(), h.lams()
    finally:
        h.close()
    err = _far(l, _reference(*t))
    print("ring 4, max_iter 3: converged %d, iterations %d, |dl| = %.3e;  then converged %d after %d more, max|l - l_ref| = %.3e"
          % (res + again[:2] + (err,)))
    assert res[:2] == (0.0, 3.0) and np.isfinite(res[2]) and res[2] > 0.0
    assert all(np.all(np.isfinite(x)) for x in mid)
    assert again[0] == 1.0 and again[2] < TOL_L and err <= NEAR


def test_the_solver_without_a_ring_agrees_with_the_default_ring(ctx):
    from libdmet_preview_amd.solver import cc_lambda
    from tests.test_gpu_cclambda import _case
    s, _, _, _, ref = _case(RUN_SHAPE[0], RUN_SHAPE[1])               # the same system after the DEVICE SCF, solved with a ring of 8
    assert ref.diis_space == 8
    obj = cc_lambda.RCCSDLambda(s.mf)
    obj.conv_tol, obj.conv_tol_normt, obj.diis_space = 1e-12, 1e-10, 0
    try:
        obj.kernel()
        l1, l2 = obj.solve_lambda()
        ok = obj.converged and obj.converged_lambda
        cycles = (obj.cycles, obj.cycles_lambda)
    finally:
        obj.close()
    err = max(np.abs(l1 - ref.l1).max(), np.abs(l2 - ref.l2).max())
    print("RCCSDLambda, diis_space 0: %d T iterations, %d Lambda sweeps (ring of 8: %d, %d);  max|l - l(ring 8)| = %.3e"
          % (cycles + (ref.cycles, ref.cycles_lambda, err)))
    assert ok and err <= NEAR
    assert cycles[1] > ref.cycles_lambda                             # plain sweeping is what ran: it takes longer than DIIS


# ---- stale state ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stale_case(o, v):
    """(Fock matrix, blocks, t_A, t_B, l) at rotated host orbitals: shared, never modified."""
    _, fock, blocks = _host(o, v, True)
    rng = np.random.default_rng(40 + o + v)
    return fock, blocks, CR.random_amplitudes(rng, o, v), CR.random_amplitudes(rng, o, v), CR.random_amplitudes(rng, o, v)


def _sweep(h, l):
    h.lambda_set(*l)
    h.lambda_update()
    return h.lams()


@pytest.mark.parametrize("how", ["set", "update", "init", "run"])
@pytest.mark.parametrize("o,v", STALE)
def test_a_sweep_after_t_changed_is_the_sweep_of_a_fresh_handle(ctx, o, v, how):
    fock, blocks, t_a, t_b, l = _stale_case(o, v)
    h = Handle(ctx, o, v, fock, blocks, diis=0)
    try:
        h.set(*t_a)
        at_a = _sweep(h, l)                                          # the kept intermediates now belong to t_A
        if how == "set":
            h.set(*t_b)
        elif how == "update":
            h.update()
        elif how == "init":
            h.init()
        else:
            assert h.run(1)[2] == 1.0
        t_now = h.amps()
        got = _sweep(h, l)
    finally:
        h.close()
    f = Handle(ctx, o, v, fock, blocks, diis=0)
    try:
        f.set(*t_now)
        want = _sweep(f, l)
    finally:
        f.close()
    print("(o, v) = (%d, %d), t changed through %s: max|t_now - t_A| = %.3e, the sweep moved by %.3e, against a fresh handle %.3e"
          % (o, v, how, _far(t_now, t_a), _far(got, at_a), _far(got, want)))
    assert _far(t_now, t_a) > 1e-3 and _far(want, at_a) > 1e-6       # a sweep on the intermediates of t_A would be seen
    assert _same(got, want)


@pytest.mark.parametrize("o,v", STALE)
def test_other_calls_between_two_sweeps_change_nothing(ctx, o, v):
    fock, blocks, t_a, _, l = _stale_case(o, v)

    def others(h):
        return (np.float64(h.energy()),) + h.residual() + (np.float64(h.lagrangian(*l)), h.rdm1())

    h = Handle(ctx, o, v, fock, blocks, diis=0)
    try:
        h.set(*t_a)
        h.lambda_set(*l)
        before = others(h)                                           # no sweep yet
        first = _sweep(h, l)
        second = _sweep(h, l)                                        # nothing in between
        h.lambda_set(*l)
        between = others(h)                                          # the work buffers of the sweep are overwritten here
        h.lambda_update()
        third = h.lams()
        h.lambda_set(*l)
        after = others(h)
    finally:
        h.close()
    assert all(np.all(np.isfinite(x)) for x in before)
    assert _same(first, second) and _same(first, third)
    assert _same(before, between) and _same(before, after)


# ---- memory --------------------------------------------------------------------------------------------------------------------
def test_lambda_memory_is_taken_once_and_given_back(ctx):
    """o = v = 24, ring of 2, random blocks (nothing is divided in what runs here): the Lambda plan is about 27 MB, far above any
    block the driver could hand out of memory it already holds.  A first round makes the context's own lazily allocated workspaces,
    which outlive a handle; the figures are taken in the second."""
    from libdmet_preview_amd._lib import lib, c_vp
    from libdmet_preview_amd.solver import cc_lambda
    o = v = 24
    plan = cc_lambda.lambda_plan_bytes(o, v, 2)
    npair = v * (v + 1) // 2
    rng = np.random.default_rng(0)
    sizes = [(o + v) ** 2, o ** 4, o ** 3 * v, o * o * v * v, o * o * v * v, o * o * v * v, o * v ** 3, npair * npair]
    dev = [ctx.to_device(0.01 * rng.standard_normal(k)) for k in sizes]
    d_t1, d_t2, d_e = ctx.to_device(0.01 * rng.standard_normal(o * v)), dev[3], ctx.empty((1,), np.float64)
    d_r1, d_r2 = ctx.empty((o, v), np.float64), ctx.empty((o, o, v, v), np.float64)

    def free_now():
        ctx.sync()
        return ctx.mem_info()[0]

    for round_ in range(2):
        start = free_now()
        h = c_vp()
        ctx.check(lib.dmk_rccsd_create(ctx.h, o, v, *([d.ptr for d in dev] + [npair, 2, C.byref(h)])))
        try:
            ctx.check(lib.dmk_rccsd_set(h, d_t1.ptr, d_t2.ptr))
            created = free_now()
            ctx.check(lib.dmk_rccsd_residual(h, d_r1.ptr, d_r2.ptr))
            ctx.check(lib.dmk_rccsd_lagrangian(h, d_t1.ptr, d_t2.ptr, d_e.ptr))
            no_lambda = free_now()
            ctx.check(lib.dmk_rccsd_lambda_set(h, d_t1.ptr, d_t2.ptr))
            first = free_now()
            ctx.check(lib.dmk_rccsd_lambda_update(h))
            ctx.check(lib.dmk_rccsd_lambda_set(h, d_t1.ptr, d_t2.ptr))
            second = free_now()
        finally:
            ctx.check(lib.dmk_rccsd_free(h))
        end = free_now()
    print("o = v = 24, ring 2: create took %d bytes, residual + lagrangian %d, the first lambda_set %d (plan %d), sweep + second "
          "lambda_set %d, after free %d below the start" % (start - created, created - no_lambda, no_lambda - first, plan, first - second,
                                                            start - end))
    assert np.isfinite(d_e.get()[0]) and np.all(np.isfinite(d_r2.get()))
    assert no_lambda == created
    assert plan <= no_lambda - first < plan + (2 << 20)
    assert second == first
    assert end == start


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_lambda_entries_refuse_bad_states_and_arguments(ctx):
    from libdmet_preview_amd._lib import lib, c_dbl
    o, v = RUN_SHAPE
    _, fock, blocks = _run_case()
    t1, t2 = CR.random_amplitudes(np.random.default_rng(5), o, v)
    h = Handle(ctx, o, v, fock, blocks, diis=2)
    try:
        d1, d2, d_e, d_g = ctx.to_device(t1), ctx.to_device(t2), ctx.empty((1,), np.float64), ctx.empty((o + v, o + v), np.float64)
        res = (c_dbl * 3)()
        # a fresh handle has no amplitudes
        assert lib.dmk_rccsd_lambda_run(h.h, 5, TOL_L, res) == DMK_ERR_STATE
        assert lib.dmk_rccsd_residual(h.h, d1.ptr, d2.ptr) == DMK_ERR_STATE
        assert lib.dmk_rccsd_lagrangian(h.h, d1.ptr, d2.ptr, d_e.ptr) == DMK_ERR_STATE
        assert lib.dmk_rccsd_lambda_init(h.h) == DMK_ERR_STATE and lib.dmk_rccsd_lambda_update(h.h) == DMK_ERR_STATE
        h.set(t1, t2)
        # amplitudes, no Lambda amplitudes
        for what in (L1, L2):
            assert lib.dmk_rccsd_get(h.h, what, d2.ptr) == DMK_ERR_STATE
        assert lib.dmk_rccsd_rdm1(h.h, d_g.ptr) == DMK_ERR_STATE
        assert lib.dmk_rccsd_lambda_update(h.h) == DMK_ERR_STATE
        assert lib.dmk_rccsd_lambda_set(h.h, None, d2.ptr) == DMK_ERR_INVALID and lib.dmk_rccsd_lambda_set(h.h, d1.ptr, None) == DMK_ERR_INVALID
        assert lib.dmk_rccsd_get(h.h, L1, d1.ptr) == DMK_ERR_STATE                      # the refused lambda_set left no l
        h.lambda_set(t1, t2)
        assert lib.dmk_rccsd_lambda_run(h.h, -1, TOL_L, res) == DMK_ERR_INVALID
        assert lib.dmk_rccsd_lambda_run(h.h, 5, TOL_L, None) == DMK_ERR_INVALID
        assert lib.dmk_rccsd_rdm1(h.h, None) == DMK_ERR_INVALID
        assert lib.dmk_rccsd_residual(h.h, None, d2.ptr) == DMK_ERR_INVALID and lib.dmk_rccsd_residual(h.h, d1.ptr, None) == DMK_ERR_INVALID
        for args in ((None, d2.ptr, d_e.ptr), (d1.ptr, None, d_e.ptr), (d1.ptr, d2.ptr, None)):
            assert lib.dmk_rccsd_lagrangian(h.h, *args) == DMK_ERR_INVALID
        assert lib.dmk_rccsd_get(h.h, L1, None) == DMK_ERR_INVALID and lib.dmk_rccsd_get(h.h, L2 + 1, d1.ptr) == DMK_ERR_INVALID
        for call in (lambda: lib.dmk_rccsd_lambda_init(None), lambda: lib.dmk_rccsd_lambda_set(None, d1.ptr, d2.ptr),
                     lambda: lib.dmk_rccsd_lambda_update(None), lambda: lib.dmk_rccsd_lambda_run(None, 5, TOL_L, res),
                     lambda: lib.dmk_rccsd_rdm1(None, d_g.ptr), lambda: lib.dmk_rccsd_residual(None, d1.ptr, d2.ptr),
                     lambda: lib.dmk_rccsd_lagrangian(None, d1.ptr, d2.ptr, d_e.ptr)):
            assert call() == DMK_ERR_INVALID
        # the refused calls changed nothing: l is what lambda_set gave, and the good calls go through
        assert _same(h.lams(), (t1, t2))
        assert lib.dmk_rccsd_rdm1(h.h, d_g.ptr) == DMK_OK and lib.dmk_rccsd_lagrangian(h.h, d1.ptr, d2.ptr, d_e.ptr) == DMK_OK
    finally:
        h.close()

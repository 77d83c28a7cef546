"""update_kernel (K4), is_weights_kernel (K5) and mode_stats_kernel against plain fp64 references of the same operations
(tests/update_oracle.py), through Engine.update / is_weights / mode_stats / cost_eval, at the shapes where the kernels take
another path: two elements per thread (M % 4 != 0) in every dtype combination, S across the 64-row ballot groups and the
256-thread strides, M beyond one pass of the element loop, 1 .. 8 rows with weight (the four-rows-in-flight loop and its
remainder) at chosen positions, P > 64 for the statistics shards; both K5 branches, with and without a goal, one and two
blocks per particle; the statistics kernel's 16-wave round-robin, its unrolled loop, the count element alone in a block,
shard offsets that cut a goal.  The bounds are derived from the kernels' arithmetic (fp64, except the fp32 subtraction
x - mu and the final rounding of each output), not measured.  Last, through Engine.step, the update whose scratch has no room
for the importance-sampling tail.  Needs the MI355X: run with `-m gpu`."""
import pytest
import torch

from tests import update_oracle as U

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS32, TINY32 = 2. ** -23, 2. ** -149


def TA(dtype):
    return {"device": DEV, "dtype": dtype}


def engine(n, T, P, S, dtype, **kw):
    from stoch_gpmp_amd.engine import Engine
    return Engine(n, T, P, S, tensor_args=TA(dtype), **kw)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def worst(err, bound):
    """max of err / bound with 0 / 0 = 0 (both fp64 CPU tensors): <= 1 means every element is within its bound."""
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    return float(r.max())


# --------------------------------------------------------------------------------------------------------------- K4
def run_update(eng, case, weights=True, grad=True, means_prev=True, stats=None):
    """One sgpmp_update from the case's inputs -> (weights, grad, means_prev, new means) device tensors (None: not asked for)."""
    real = case["real"]
    P, S, T, d = case["samples"].shape
    means = case["means"].to(DEV).clone()
    sentinel = 12345.0
    w = torch.full((P, S), sentinel, **TA(real)) if weights else None
    g = torch.full((P, T, d), sentinel, **TA(real)) if grad else None
    mp = torch.full((P, T, d), sentinel, **TA(real)) if means_prev else None
    eng.update(case["costs"].to(DEV), case["samples"].to(DEV), means, case["tau"], case["step"], weights=w, grad=g,
               means_prev=mp, stats=stats)
    torch.cuda.synchronize()
    return w, g, mp, means


@pytest.mark.parametrize("dtype_name", list(U.UPDATE_DTYPES))
@pytest.mark.parametrize("shape", U.UPDATE_SHAPES, ids=[f"n{n}-T{T}-P{P}-S{S}" for n, T, P, S in U.UPDATE_SHAPES])
def test_update_matches_fp64_softmax_reference(shape, dtype_name):
    n, T, P, S = shape
    real = U.UPDATE_DTYPES[dtype_name][0]
    eng = engine(n, T, P, S, real)
    for regime in U.update_regimes(S):
        name = regime[0]
        case = U.update_case(shape, dtype_name, regime)
        tau, step = case["tau"], case["step"]
        w_ref, g_ref, mu_ref, A = U.update_reference(case["costs"], case["samples"], case["means"], tau, step)
        # the reference alone: the case is the case it claims to be
        assert (w_ref != 0).sum(1).tolist() == [case["expect"]] * P, name
        assert float(A.max()) > 0, name

        stats = torch.zeros(64, 4, device=DEV, dtype=torch.float64)
        w, g, mp, mu = run_update(eng, case, stats=stats)
        wd, gd, mud = w.double().cpu(), g.double().cpu(), mu.double().cpu()
        if real == torch.float64:
            bw = 1e-11 * w_ref.abs() + 1e-300
            bg = 1e-10 * A + 1e-14
            bm = 1e-12 * mu_ref.abs() + step * 1e-10 * A
        else:
            bw = EPS32 * w_ref.abs() + TINY32
            bg = 2. ** -22 * A
            bm = EPS32 * mu_ref.abs() + step * 2. ** -22 * A
        rw, rg, rm = worst((wd - w_ref).abs(), bw), worst((gd - g_ref).abs(), bg), worst((mud - mu_ref).abs(), bm)
        print(f"{name}: weights {rw:.3g}, grad {rg:.3g}, means {rm:.3g} of their bounds")
        assert bool(torch.isfinite(gd).all()) and bool(torch.isfinite(mud).all()), name
        assert rw <= 1, (name, "weights", rw)
        assert rg <= 1, (name, "grad", rg)
        assert rm <= 1, (name, "means", rm)
        assert same_bits(mp.cpu(), case["means"]), (name, "means_prev")

        # statistics: (sum of all costs, sum over particles of the smallest cost, particles), in 64 shards by p & 63; accumulated
        tot, mins, cnt, per_shard = U.stats_reference(case["costs"])
        st = stats.cpu()
        assert bool((st[:, 3] == 0).all())
        assert abs(float(st[:, 0].sum()) - tot) <= 1e-12 * abs(tot), (name, float(st[:, 0].sum()), tot)
        assert abs(float(st[:, 1].sum()) - mins) <= 1e-12 * abs(mins), (name, float(st[:, 1].sum()), mins)
        assert st[:, 2].tolist() == per_shard.tolist() and float(st[:, 2].sum()) == cnt, name

        # the same inputs again, into the same statistics buffer: the same bits, and twice the statistics
        w2, g2, mp2, mu2 = run_update(eng, case, stats=stats)
        assert same_bits(w2, w) and same_bits(g2, g) and same_bits(mp2, mp) and same_bits(mu2, mu), (name, "second call")
        st2 = stats.cpu()
        assert st2[:, 2].tolist() == (2 * per_shard).tolist(), name
        assert abs(float(st2[:, 0].sum()) - 2 * tot) <= 1e-12 * abs(2 * tot), name
        assert abs(float(st2[:, 1].sum()) - 2 * mins) <= 1e-12 * abs(2 * mins), name

        # each optional output left out: the others and the new means keep their bits
        for skip in ("weights", "grad", "means_prev"):
            wo, go, mpo, muo = run_update(eng, case, **{skip: False})
            assert same_bits(muo, mu), (name, skip, "means")
            for got, full, tag in ((wo, w, "weights"), (go, g, "grad"), (mpo, mp, "means_prev")):
                if tag == skip:
                    assert got is None
                else:
                    assert same_bits(got, full), (name, "without " + skip, tag)
    eng.close()


# --------------------------------------------------------------------------------------------------------------- K5
def isw_engine(case, P, S, dtype):
    from stoch_gpmp_amd import _lib as L
    n, T, dt, ss, sg, sgoal = case
    eng = engine(n, T, P, S, dtype)
    eng.set_prior(L.PRIOR_SAMPLE, dt, ss, sg, sgoal, Q_c_inv=U.isw_prior(case)[0])
    return eng


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("case", U.ISW_CASES, ids=[U.isw_case_id(c) for c in U.ISW_CASES])
def test_is_weights_match_the_dense_precision(case, dtype):
    n, T = case[0], case[1]
    Sigma_inv = U.isw_prior(case)[4]
    eng = isw_engine(case, 3, 1, dtype)
    for P in (1, 3):
        means = U.isw_means(case, P, dtype)
        for tau in (1., 3.):
            ref = U.isw_reference(case, means, tau, Sigma_inv)
            out = torch.full((P, T + 1, 2 * n), 777.0, **TA(dtype))
            got = eng.is_weights(means.to(DEV), tau, out=out)
            torch.cuda.synchronize()
            assert got.dtype == dtype
            got = got.double().cpu()
            assert bool((got[:, T] == 0).all()), "spare block T"
            scale = ref.abs().amax((1, 2), keepdim=True)
            assert float(scale.min()) > 0
            bound = 1e-12 * scale if dtype == torch.float64 else EPS32 * ref.abs() + 1e-12 * scale
            r = worst((got - ref).abs(), bound.expand_as(ref))
            print(f"P={P} tau={tau}: {r:.3g} of the bound")
            assert r <= 1, (P, tau, r)
            again = eng.is_weights(means.to(DEV), tau)
            torch.cuda.synchronize()
            assert torch.equal(again.double().cpu(), got)
    eng.close()


@pytest.mark.parametrize("case", U.ISW_CONSUMER_CASES, ids=[U.isw_case_id(c) for c in U.ISW_CONSUMER_CASES])
def test_sweep_with_is_weights_adds_the_dense_is_term(case):
    """What the weights are for: cost_eval with them minus cost_eval without is tau x^T Sigma^-1 mu, Sigma^-1 the dense
    precision of the oracle (same one-term program on both sides: a GP factor of the prior's time step)."""
    from stoch_gpmp_amd import _lib as L
    n, T, dt, ss, sg, sgoal = case
    P, S, tau = 3, 3, 3.
    Sigma_inv = U.isw_prior(case)[4]
    eng = isw_engine(case, P, S, torch.float64)
    eng.set_costs([dict(kind=L.COST_GP, flags=0, sigma=1.0 if sg is None else sg, dt=dt)])
    means = U.isw_means(case, P, torch.float64)
    g = torch.Generator().manual_seed(17)
    x = torch.randn(P, S, T, 2 * n, generator=g, dtype=torch.float64)
    xd = x.to(DEV).contiguous()
    isw = eng.is_weights(means.to(DEV), tau)
    with_is = eng.cost_eval(xd, is_weights=isw, rows_per_particle=S, out64=torch.empty(P * S, device=DEV, dtype=torch.float64))
    plain = eng.cost_eval(xd, out64=torch.empty(P * S, device=DEV, dtype=torch.float64))
    torch.cuda.synchronize()
    diff = (with_is - plain).cpu().reshape(P, S)
    want = U.is_term_reference(Sigma_inv, x, means, tau)
    rel = float(((diff - want).abs() / want.abs()).max())
    print(f"IS term through the sweep: {rel:.3g} relative")
    assert float(plain.abs().min()) > 0
    assert rel <= 1e-9, rel
    eng.close()


# ------------------------------------------------------------------------------------------------- mode statistics
def mode_stats_once(n, T, G, nppg, Pg, off, P, means, dtype, out=None):
    eng = engine(n, T, P, 1, dtype, num_goals=G, num_particles_per_goal=nppg, particle_offset=off, num_particles_global=Pg)
    dev_means = means[off:off + P].contiguous().to(DEV)
    got = eng.mode_stats(dev_means, out=out)
    again = eng.mode_stats(dev_means)
    torch.cuda.synchronize()
    assert same_bits(got, again), "two calls"
    eng.close()
    return got.cpu()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("n,T", U.MODE_STATS_ELEMENTS)
def test_mode_stats_match_per_goal_fp64_sums(n, T, dtype):
    M = T * 2 * n
    unsharded = {}
    for G, nppg, Pg, shards in U.MODE_STATS_LAYOUTS:
        tag = (G, nppg, Pg, len(shards))
        means = U.mode_stats_means(n, T, Pg, dtype)
        full_ref, full_scale = U.mode_stats_reference(means, G, nppg)
        total = torch.zeros(G, M + 1, 2, dtype=torch.float64)
        for off, P in shards:
            # (a buffer full of a finite sentinel: the entry point zeroes it before the kernel accumulates)
            out = torch.full((G, M + 1, 2), -3.25e7, device=DEV, dtype=torch.float64)
            got = mode_stats_once(n, T, G, nppg, Pg, off, P, means, dtype, out=out)
            ref, scale = U.mode_stats_reference(means[off:off + P], G, nppg, off)
            assert got.shape == (G, M + 1, 2)
            assert got[:, M, 0].tolist() == ref[:, M, 0].tolist(), (tag, off, "counts")
            assert bool((got[:, M, 1] == 0).all()), (tag, off)
            r = worst((got[:, :M] - ref[:, :M]).abs(), 1e-13 * scale[:, :M])
            print(f"G={G} nppg={nppg} shard ({off}, {P}): {r:.3g} of the bound")
            assert r <= 1, (tag, off, r)
            total += got
        assert total[:, M, 0].tolist() == full_ref[:, M, 0].tolist(), tag
        assert worst((total[:, :M] - full_ref[:, :M]).abs(), 1e-13 * full_scale[:, :M]) <= 1, tag
        if len(shards) == 1:
            unsharded[(G, nppg, Pg)] = total
        elif (G, nppg, Pg) in unsharded:               # the shards' outputs add up to the unsharded run's
            one = unsharded[(G, nppg, Pg)]
            assert total[:, M, 0].tolist() == one[:, M, 0].tolist(), tag
            assert worst((total[:, :M] - one[:, :M]).abs(), 1e-13 * full_scale[:, :M]) <= 1, tag
    assert (3, 17, 51) in unsharded


# ------------------------------------------------------------------------------------------ the step's update without its tail
def two_steps(S, kept):
    """Two sgpmp_step calls of a planar fp32 GP-cost problem, n = 2, T = 160, P = 2, S samples; the second with
    SGPMP_STEP_MEANS_KEPT if `kept` -> (means, costs, statistics after each step, launches of the second step)."""
    from stoch_gpmp_amd import _lib as L
    n, T, P, dt = 2, 160, 2, 0.02
    real, d = torch.float32, 2 * n
    eng = engine(n, T, P, S, real)
    try:
        eng.set_prior(L.PRIOR_SAMPLE, dt, 1e-3, 20.0, 1e-3)
        eng.set_costs([dict(kind=L.COST_GP, flags=0, sigma=20.0, dt=dt)])
        means = U.isw_means((n, T, dt, 1e-3, 20.0, 1e-3), P, real).to(DEV)
        out = []
        for it in range(2):
            samples, costs = torch.zeros(P, S, T, d, **TA(real)), torch.zeros(P, S, **TA(real))
            stats = torch.zeros(64, 4, device=DEV, dtype=torch.float64)
            eng.step(23, 2 + it, means, samples, 3.0, 0.5, costs=costs, stats=stats, flags=L.STEP_MEANS_KEPT if it and kept else 0)
            torch.cuda.synchronize()
            out += [means.clone().cpu(), costs.cpu(), stats.cpu()]
        return out, eng.last_step_launches()
    finally:
        eng.close()


def test_step_whose_update_has_no_room_for_the_tail_computes_the_next_weights_itself():
    """Scratch of one particle's update, fp32, n = 2, T = 160: 12 S bytes of weights and indices, then the M * 4 = 2560 bytes of
    new means the importance-sampling tail reads.  S = 5184: 62 208 + 2560 + the 256-byte reserve = 65 024 <= 65 536, the tail
    runs and a step that keeps the means skips the weights launch.  S = 5248: 62 976 + 2560 + 256 = 65 792, the tail is
    dropped (62 976 + update_kernel's 1072 bytes of static LDS = 64 048 still fit a workgroup): the update must say so, and
    the next step must compute its weights with a launch of its own although told the means were kept -- everything it returns
    equal, bit for bit, to the same two steps without the flag, with one launch more than at S = 5184."""
    flagged, launches = two_steps(5248, True)
    plain, launches_plain = two_steps(5248, False)
    for i, (x, y) in enumerate(zip(flagged, plain)):
        assert same_bits(x, y), i
    assert bool(torch.isfinite(flagged[3]).all()) and not torch.equal(flagged[0], flagged[3])    # the second step moved the means
    assert float(flagged[4].abs().max()) > 0 and float(flagged[5][:, 2].sum()) == 2
    _, launches_tail = two_steps(5184, True)
    assert launches == launches_tail + 1, (launches, launches_tail)
    assert launches_plain == launches, (launches_plain, launches)

"""The stand-alone trajectory samplers (csrc/sampler.hip) against the fp64 oracle at every branch of their host dispatch
(sample_dispatch): sample_iso_kernel, sample_iso_small_kernel and sample_dense_kernel, both precisions.  Every case first asserts
which kernel ran and how it was launched (Engine.last_sample_kernel) against a LITERAL string -- derived by hand from the
dispatch rule, not from a Python copy of it -- and then the values.  Needs the MI355X: run with `-m gpu`.

Dispatch facts the literals rest on (n dof, d = 2 n, T waypoints, S samples, `modes` particles):
  * isotropic prior, main kernel: spw = 64 / n samples per wave, waves = ceil(S / spw) per mode, up to four waves per workgroup;
    fp64 stores two elements per lane (VW=2), fp32 four when T d 4 bytes is a multiple of 16 -- T n even -- and two otherwise;
    a row of a 16-waypoint chunk is seg = tc d / VW vectors, flushed by lpr = min(64, pow2 >= 16 d / VW) lanes: one vector per lane
    when seg <= lpr (`one_j`), a loop otherwise;
  * native noise and waves x modes < 256 (unless the option no_small_sampler): the few-wave kernel, dof count compiled in for
    n = 2, 3, 7 (NC, else 0), chunks of tc = 64 waypoints when T > 32 and of 32 otherwise, spb = 8 samples per workgroup -- in
    fp64 4 while ceil(S / 4) x modes <= 512;
  * a full Q_c^-1 or per-mode precisions: the dense kernel, one wave per 16 samples, four waves per workgroup.
The observed errors of one run are on record in profiles/r18/sampler_oracle.txt."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_equiv as R
from oracle.native_noise import native_eps

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
DTYPES = [pytest.param(F64, id="f64"), pytest.param(F32, id="f32")]
# the project's own bounds (test_gpu_kernels.py: test_sampler_external_eps_matches_oracle, the dense sampler tests), on
# |out - ref| <= rtol |ref| + rtol max|ref - means|
RTOL = {F64: 1e-8, F32: 2e-4}
DT, SS, SG, SGOAL = 0.1, 0.3, 1.0, 0.4                   # the isotropic prior of every case
SEED, DRAW, OFF = 0x1234567887654321, 77, 5              # 64-bit seed with both halves non-zero; first global particle

ISO2, ISO4 = "sample_iso_kernel<VW=2>", "sample_iso_kernel<VW=4>"
DENSE, DENSE_PM = "sample_dense_kernel", "sample_dense_kernel(per-mode)"


def small(nc, spb, tc):
    return f"sample_iso_small_kernel<NC={nc},spb={spb},tc={tc}>"


def TA(dtype):
    return {"device": DEV, "dtype": dtype}


def engine(n, T, P, S, dtype):
    from stoch_gpmp_amd.engine import Engine
    return Engine(n, T, P, S, tensor_args=TA(dtype))


def iso_engine(n, T, P, S, dtype):
    from stoch_gpmp_amd import _lib as L
    eng = engine(n, T, P, S, dtype)
    eng.set_prior(L.PRIOR_SAMPLE, DT, SS, SG, SGOAL)
    return eng


def draw(eng, means, S, seed=SEED, draw=DRAW, **kw):
    from stoch_gpmp_amd import _lib as L
    return eng.sample(L.PRIOR_SAMPLE, seed, draw, means, S, **kw)


def rand_means(modes, T, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(modes, T, d, generator=g, dtype=F64)


# ---- the oracle: oracle.ref_equiv.TrajPrior (torch's MultivariateNormal on the dense precision), built once per shape with zero
# means and shared -- TrajPrior.sample(S, eps) is then scale_tril @ eps, and the case adds its own means
@functools.lru_cache(maxsize=None)
def iso_oracle(n, T, modes):
    d = 2 * n
    return R.TrajPrior(T, n, DT, R.unary_K(d, SS, F64), R.q_inv_matrix(n, DT, SG, F64), torch.zeros(d, dtype=F64),
                       means=torch.zeros(modes, T, d, dtype=F64), K_g=R.unary_K(d, SGOAL, F64),
                       goals=torch.zeros(modes, d, dtype=F64))


DENSE_DT, DENSE_SS, DENSE_SGOAL = 0.1, 0.05, 0.2         # (as test_dense_sampler_with_full_Qc_matches_oracle)


@functools.lru_cache(maxsize=None)
def full_Qc_inv(n):
    g = torch.Generator().manual_seed(3)
    A = torch.randn(n, n, generator=g, dtype=F64)
    return A @ A.t() + n * torch.eye(n, dtype=F64)


@functools.lru_cache(maxsize=None)
def dense_oracle(n, T, modes):
    d = 2 * n
    return R.TrajPrior(T, n, DENSE_DT, R.unary_K(d, DENSE_SS, F64), R.q_inv_matrix(n, DENSE_DT, None, F64, Q_c_inv=full_Qc_inv(n)),
                       torch.zeros(d, dtype=F64), means=torch.zeros(modes, T, d, dtype=F64), K_g=R.unary_K(d, DENSE_SGOAL, F64),
                       goals=torch.zeros(modes, d, dtype=F64))


def reference(prior, means, eps):
    """[modes, S, T, d] in fp64: means + scale_tril @ eps of the oracle's dense distribution."""
    return means.unsqueeze(1) + prior.sample(eps.shape[0], eps=eps)


def native(eng, dtype, n, T, particles, S):
    """The eps the kernels draw for the GLOBAL particles `particles` and samples 0 .. S: the CPU restatement of the stream; in an
    fp64 context the library's own read-back of it, first held to the restatement (test_native_noise_samples_match_the_restated_
    stream's rule: the restatement follows the hardware's log2 / sin / cos to an ulp of fp32, the fp64 sampler is held to 1e-8)."""
    from stoch_gpmp_amd import _lib as L
    particles = list(particles)
    eps = torch.from_numpy(native_eps(SEED, DRAW, particles, S, T, n, "float64" if dtype == F64 else "float32",
                                      rounds=int(L.load().sgpmp_philox_rounds()))).double()
    if dtype == F64:
        lo = min(particles)
        dev_eps = eng.noise(SEED, DRAW, max(particles) + 1 - lo, S, mode_offset=lo).cpu()[:, [p - lo for p in particles]]
        assert float((dev_eps - eps).abs().max()) < 2e-6
        eps = dev_eps.contiguous()
    return eps


def check(out, ref, means, dtype, what):
    out, scale = out.double().cpu(), float((ref - means.unsqueeze(1)).abs().max())
    assert out.shape == ref.shape, (out.shape, ref.shape)
    print(f"sampler_oracle {what} {'fp64' if dtype == F64 else 'fp32'}: max|out - ref| / max|ref - means| = "
          f"{float((out - ref).abs().max()) / scale:.3e}")
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=RTOL[dtype], atol=RTOL[dtype] * scale)


# ------------------------------------------------------------------------------------------- (a), (b): sample_iso_kernel
MAIN_CASES = [  # n, T, S, fp32 launch, fp64 launch
    # spw 64: three waves in one workgroup, two rows in the last.  fp32: VW=4, lpr 8 (lpr_shift 3), seg 8 -- fp64: lpr 16, seg 16
    (1, 16, 130, ISO4, ISO2),
    # T n odd: fp32 VW=2 with lpr 16; one short chunk (tc 5, seg 5); two waves, six rows in the second
    (1, 5, 70, ISO2, ISO2),
    # spw 16: five waves = two workgroups, the second with one live (six rows) and three dead waves (rows <= 0).  fp64: seg 64 ==
    # lpr 64, exactly the one_j boundary, in the full chunk and seg 32 in the short one (tc 8); fp32 VW=4: lpr 32, seg 32 / 16
    (4, 24, 70, ISO4, ISO2),
    # spw 12, four slack lanes; T n odd: VW=2 in both precisions, seg 80 > lpr 64: looped flush with a ragged second trip
    # (16 of 64 lanes); the last chunk (tc 3, seg 15) switches to one_j inside the launch; three waves, three rows in the last
    (5, 19, 27, ISO2, ISO2),
    # spw 10, four slack lanes.  fp32 VW=4: seg 48 <= lpr 64, one_j with idle lanes -- fp64: seg 96, looped; last chunk tc 1
    # (seg 3 / 6: one_j in both); three waves, one row in the last
    (6, 33, 21, ISO4, ISO2),
    # spw 9, one slack lane; T n odd: VW=2, seg 112 looped, last chunk tc 1 (seg 7) one_j; five waves = two workgroups, the second
    # with one live wave (four rows) and three dead ones
    (7, 17, 40, ISO2, ISO2),
    # spw 8, no slack lane; two waves, one row in the second.  fp32 VW=4: seg 64 == lpr 64 (one_j boundary) -- fp64: seg 128, two
    # full trips of the looped flush; T == one chunk exactly
    (8, 16, 9, ISO4, ISO2),
    # nine chunks, the last with tc 2; spw 32: the third wave holds one row
    (2, 130, 65, ISO4, ISO2),
    # T < 16: one short chunk (tc 6; fp32 VW=4 seg 9 of lpr 32, fp64 seg 18 of lpr 64); spw 21, one slack lane; the second wave
    # holds one row
    (3, 6, 22, ISO4, ISO2),
]
MAIN_IDS = [f"n{c[0]}-T{c[1]}-S{c[2]}" for c in MAIN_CASES]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,T,S,k32,k64", MAIN_CASES, ids=MAIN_IDS)
def test_main_kernel_with_external_eps_matches_oracle(n, T, S, k32, k64, dtype):
    """eps of modes + 2 modes read at eps_mode_offset = 1: an indexing slip reads another mode's noise."""
    d, modes = 2 * n, 2
    means = rand_means(modes, T, d, 100 + n)
    g = torch.Generator().manual_seed(200 + T)
    eps = torch.randn(S, modes + 2, T * d, generator=g, dtype=F64)
    ref = reference(iso_oracle(n, T, modes), means, eps[:, 1:1 + modes].contiguous())
    eng = iso_engine(n, T, modes, S, dtype)
    out = draw(eng, means.to(**TA(dtype)), S, seed=0, draw=0, eps=eps.to(**TA(dtype)), eps_mode_offset=1)
    assert eng.last_sample_kernel() == (k64 if dtype == F64 else k32)
    check(out, ref, means, dtype, f"sample_iso_kernel external (n, T, S) = ({n}, {T}, {S})")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,T,S,k32,k64", MAIN_CASES, ids=MAIN_IDS)
def test_main_kernel_with_native_noise_matches_oracle(n, T, S, k32, k64, dtype):
    """The same launches drawing their own noise (the option no_small_sampler -- read at every call -- keeps these few-wave shapes
    on the main kernel): the two-waypoint Philox trips, the odd tail of an odd chunk, the key (seed, draw, GLOBAL particle)."""
    d, modes = 2 * n, 2
    means = rand_means(modes, T, d, 300 + n)
    eng = iso_engine(n, T, modes, S, dtype)
    eng.set_option("no_small_sampler")
    ref = reference(iso_oracle(n, T, modes), means, native(eng, dtype, n, T, range(OFF, OFF + modes), S))
    out = draw(eng, means.to(**TA(dtype)), S, mode_offset=OFF)
    assert eng.last_sample_kernel() == (k64 if dtype == F64 else k32)
    check(out, ref, means, dtype, f"sample_iso_kernel native (n, T, S) = ({n}, {T}, {S})")


# ------------------------------------------------------------------------------------------- (c): sample_iso_small_kernel
SMALL_CASES = [  # n, T, S, modes, fp32 launch, fp64 launch, what the main kernel is for the same call (fp32; fp64 is VW=2)
    # 1: NC=2, tc 32: one short odd chunk (tc 9, the last block half used); 11 samples: the last workgroup partly filled
    (2, 9, 11, 3, small(2, 8, 32), small(2, 4, 32), ISO4),
    # 2: NC=3; T = 32 is not > 32: one FULL chunk of tc 32
    (3, 32, 11, 3, small(3, 8, 32), small(3, 4, 32), ISO4),
    # 3: NC=7, tc 64: one short odd chunk (tc 33: the serial phase runs 48 steps, 15 of them past the chunk)
    (7, 33, 11, 3, small(7, 8, 64), small(7, 4, 64), ISO2),
    # 4: two chunks at tc 64, the second with tc 6: the state carried across a chunk boundary
    (7, 70, 11, 3, small(7, 8, 64), small(7, 4, 64), ISO4),
    # 5: three chunks, the last with tc 2
    (2, 130, 11, 3, small(2, 8, 64), small(2, 4, 64), ISO4),
    # 6 - 9: NC=0, the dof count at run time: n = 1 (one chain per sample; 70 samples: the last workgroup holds six, fp64 two),
    # 4, 8 (the widest rows: 16 reals per waypoint) and 5
    (1, 40, 70, 3, small(0, 8, 64), small(0, 4, 64), ISO4),
    (4, 16, 9, 3, small(0, 8, 32), small(0, 4, 32), ISO4),
    (8, 64, 5, 3, small(0, 8, 64), small(0, 4, 64), ISO4),
    (5, 35, 13, 3, small(0, 8, 64), small(0, 4, 64), ISO2),
    # 10: fp64 ceil(33 / 4) x 70 = 630 > 512 workgroups of four samples: spb 8; waves 2 x 70 = 140 < 256 keeps the small kernel
    (2, 8, 33, 70, small(2, 8, 32), small(2, 8, 32), ISO4),
    # 11: the same shape with three modes: fp64 spb 4
    (2, 8, 33, 3, small(2, 8, 32), small(2, 4, 32), ISO4),
]
SMALL_IDS = [f"{i + 1}-n{c[0]}-T{c[1]}-S{c[2]}-m{c[3]}" for i, c in enumerate(SMALL_CASES)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,T,S,modes,k32,k64,main32", SMALL_CASES, ids=SMALL_IDS)
def test_small_kernel_matches_oracle(n, T, S, modes, k32, k64, main32, dtype):
    d = 2 * n
    means = rand_means(modes, T, d, 400 + n)
    eng = iso_engine(n, T, modes, S, dtype)
    ref = reference(iso_oracle(n, T, modes), means, native(eng, dtype, n, T, range(OFF, OFF + modes), S))
    out = draw(eng, means.to(**TA(dtype)), S, mode_offset=OFF)
    assert eng.last_sample_kernel() == (k64 if dtype == F64 else k32)
    check(out, ref, means, dtype, f"sample_iso_small_kernel (n, T, S, modes) = ({n}, {T}, {S}, {modes})")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("modes,k32,k64", [
    # one wave per mode: 255 waves < 256 -> the small kernel (fp64: ceil(8 / 4) x 255 = 510 <= 512 workgroups: spb 4)
    (255, small(2, 8, 32), small(2, 4, 32)),
    # 256 waves: the main kernel (T n = 16 even: fp32 VW=4)
    (256, ISO4, ISO2),
])
def test_small_kernel_selection_boundary_matches_oracle(modes, k32, k64, dtype):
    """(n, T, S) = (2, 8, 8): waves x modes = 255 takes the few-wave kernel, 256 the main one; first, last and two modes in between
    against the oracle."""
    n, T, S = 2, 8, 8
    d = 2 * n
    pick = [0, 85, 170, modes - 1]
    means = rand_means(modes, T, d, 500)
    eng = iso_engine(n, T, modes, S, dtype)
    ref = reference(iso_oracle(n, T, len(pick)), means[pick], native(eng, dtype, n, T, [OFF + m for m in pick], S))
    out = draw(eng, means.to(**TA(dtype)), S, mode_offset=OFF)
    assert eng.last_sample_kernel() == (k64 if dtype == F64 else k32)
    assert out.shape == (modes, S, T, d)
    check(out[pick], ref, means[pick], dtype, f"selection boundary, {modes} modes")


# ------------------------------------------------------------------------------------------- (d): bit identities
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,T,S,modes,k32,k64,main32", SMALL_CASES, ids=SMALL_IDS)
def test_small_kernel_equals_main_kernel_bitwise(n, T, S, modes, k32, k64, main32, dtype):
    """sampler.hip and DESIGN.md: same counter layout, same recurrence expressions (rng.h: scan_step is scan_step_noise followed
    by scan_step_state, every product-sum an explicit fma) -- the two isotropic kernels return identical samples."""
    means = rand_means(modes, T, 2 * n, 600 + n).to(**TA(dtype))
    eng = iso_engine(n, T, modes, S, dtype)
    a = draw(eng, means, S, mode_offset=OFF)
    assert eng.last_sample_kernel() == (k64 if dtype == F64 else k32)
    eng.set_option("no_small_sampler")
    b = draw(eng, means, S, mode_offset=OFF)
    assert eng.last_sample_kernel() == (ISO2 if dtype == F64 else main32)
    assert torch.equal(a, b), f"{int((a != b).sum())} of {a.numel()} elements differ, max {float((a - b).abs().max()):.3e}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,T,S_big,k32,k64,main32", [
    # spw 9: 86 waves x 3 modes = 258 >= 256; T n odd: fp32 VW=2
    (7, 33, 774, small(7, 8, 64), small(7, 4, 64), ISO2),
    # spw 32: 86 waves (the last with one row) x 3 modes = 258 >= 256
    (2, 70, 2721, small(2, 8, 64), small(2, 4, 64), ISO4),
])
def test_first_samples_do_not_depend_on_how_many_are_drawn(n, T, S_big, k32, k64, main32, dtype):
    """Prefix invariance across the two kernels: S = 11 takes the few-wave kernel, S_big the main kernel by itself; sample s of
    mode m is a function of (seed, draw, m, s) alone."""
    modes, S = 3, 11
    means = rand_means(modes, T, 2 * n, 700 + n).to(**TA(dtype))
    eng = iso_engine(n, T, modes, S_big, dtype)
    a = draw(eng, means, S, mode_offset=OFF)
    assert eng.last_sample_kernel() == (k64 if dtype == F64 else k32)
    b = draw(eng, means, S_big, mode_offset=OFF)
    assert eng.last_sample_kernel() == (ISO2 if dtype == F64 else main32)
    assert torch.equal(a, b[:, :S])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("no_small,k32,k64", [
    # (4, 24, 70): the main kernel's launch with dead waves -- the shard's grid is two workgroups x two modes
    (True, ISO4, ISO2),
    # the same shape on the few-wave kernel: NC=0, tc 32 (fp64: 18 x 3 workgroups: spb 4)
    (False, small(0, 8, 32), small(0, 4, 32)),
])
def test_samples_do_not_depend_on_the_shard(no_small, k32, k64, dtype):
    """Modes [1, 3) sampled alone with mode_offset = 1 are rows 1 and 2 of the unsharded call."""
    n, T, S, modes = 4, 24, 70, 3
    means = rand_means(modes, T, 2 * n, 800).to(**TA(dtype))
    eng = iso_engine(n, T, modes, S, dtype)
    if no_small:
        eng.set_option("no_small_sampler")
    whole = draw(eng, means, S)
    assert eng.last_sample_kernel() == (k64 if dtype == F64 else k32)
    shard = draw(eng, means[1:].contiguous(), S, mode_offset=1)
    assert eng.last_sample_kernel() == (k64 if dtype == F64 else k32)
    assert torch.equal(shard, whole[1:])


# ------------------------------------------------------------------------------------------- (e): sample_dense_kernel
DENSE_CASES = [  # n, T, S: a wave is a [16 state rows x 16 samples] tile, four waves per workgroup
    (1, 7, 15), (1, 7, 16), (1, 7, 17),      # state block 2 of 16 rows; last tile short by one / full / a second wave with one sample
    (8, 5, 63), (8, 5, 64), (8, 5, 65),      # state block all 16 rows; last wave short by one / one full workgroup / a second one
    (5, 9, 33),                              # state block 10 rows: rows 10 .. 15 of the accumulator maps (fp32 4 q + r, fp64 q + 4 r) idle
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("noise", ["external", "native"])
@pytest.mark.parametrize("n,T,S", DENSE_CASES)
def test_dense_kernel_tile_edges_match_oracle(n, T, S, noise, dtype):
    """Shared closed-form factors of a full random SPD Q_c^-1."""
    from stoch_gpmp_amd import _lib as L
    d, modes = 2 * n, 2
    means = rand_means(modes, T, d, 900 + n)
    eng = engine(n, T, modes, S, dtype)
    eng.set_prior(L.PRIOR_SAMPLE, DENSE_DT, DENSE_SS, None, DENSE_SGOAL, Q_c_inv=full_Qc_inv(n))
    if noise == "external":
        g = torch.Generator().manual_seed(1000 + S)
        eps = torch.randn(S, modes + 2, T * d, generator=g, dtype=F64)
        out = draw(eng, means.to(**TA(dtype)), S, seed=0, draw=0, eps=eps.to(**TA(dtype)), eps_mode_offset=1)
        eps = eps[:, 1:1 + modes].contiguous()
    else:
        eps = native(eng, dtype, n, T, range(3, 3 + modes), S)
        out = draw(eng, means.to(**TA(dtype)), S, mode_offset=3)
    assert eng.last_sample_kernel() == DENSE
    check(out, reference(dense_oracle(n, T, modes), means, eps), means, dtype, f"sample_dense_kernel {noise} (n, T, S) = ({n}, {T}, {S})")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n,T,S", [(3, 7, 17), (8, 4, 65)])
def test_dense_kernel_with_per_mode_factors_matches_torch(n, T, S, dtype):
    """Per-mode block-tridiagonal precisions (Engine.set_prior_blocks, what MultiMPPrior.set_Sigma_invs calls; built as
    test_multi_mp_prior_log_prob_and_per_mode_precisions_match_torch builds them) against loc + scale_tril @ eps of torch's
    MultivariateNormal on the dense matrices: external eps, native noise, and the refusal of a mode without factors."""
    from torch.distributions import MultivariateNormal
    from stoch_gpmp_amd import _lib as L
    dt, ss, sg, sgoal, modes = 0.1, 0.3, 0.8, 0.5, 3
    d, M = 2 * n, 2 * n * T
    g = torch.Generator().manual_seed(11 + n)
    means = torch.randn(modes + 1, T, d, generator=g, dtype=F64)
    ora = R.TrajPrior(T, n, dt, R.unary_K(d, ss, F64), R.q_inv_matrix(n, dt, sg, F64), torch.zeros(d, dtype=F64),
                      K_g=R.unary_K(d, sgoal, F64), goals=torch.zeros(1, d, dtype=F64))
    new = torch.zeros(modes, M, M, dtype=F64)
    for m in range(modes):
        A = torch.randn(T, d, d, generator=g, dtype=F64) * 0.7
        bump = torch.block_diag(*[a @ a.t() for a in A])
        new[m] = ora.Sigma_inv * (1. + 0.4 * m) + bump
    blocks = new.reshape(modes, T, d, T, d).permute(0, 1, 3, 2, 4)                      # [m, ti, tj, d, d]
    idx = torch.arange(T)
    eng = engine(n, T, modes + 1, S, dtype)
    eng.set_prior(L.PRIOR_SAMPLE, dt, ss, sg, sgoal)
    eng.set_prior_blocks(L.PRIOR_SAMPLE, blocks[:, idx, idx], blocks[:, idx[1:], idx[:-1]])
    mvn = MultivariateNormal(means[:modes].reshape(modes, M), precision_matrix=new)

    def want(eps):                                                                      # eps [S, modes, M] -> [modes, S, T, d]
        x = mvn.loc + torch.matmul(mvn._unbroadcasted_scale_tril, eps.unsqueeze(-1)).squeeze(-1)
        return x.view(S, modes, T, d).transpose(0, 1)

    mu = means[:modes].to(**TA(dtype)).contiguous()
    eps = torch.randn(S, modes + 2, M, generator=g, dtype=F64)
    out = draw(eng, mu, S, seed=0, draw=0, eps=eps.to(**TA(dtype)), eps_mode_offset=1)
    assert eng.last_sample_kernel() == DENSE_PM
    check(out, want(eps[:, 1:1 + modes].contiguous()), means[:modes], dtype, f"sample_dense_kernel(per-mode) external (n, T, S) = ({n}, {T}, {S})")
    # native noise: the noise key is the GLOBAL particle (mode_offset + m), the factor is mode m's
    eps = native(eng, dtype, n, T, range(3, 3 + modes), S)
    out = draw(eng, mu, S, mode_offset=3)
    assert eng.last_sample_kernel() == DENSE_PM
    check(out, want(eps), means[:modes], dtype, f"sample_dense_kernel(per-mode) native (n, T, S) = ({n}, {T}, {S})")
    # a fourth mode with three factor modes: refused (sample_dispatch: hipErrorInvalidValue), nothing launched
    with pytest.raises(L.SgpmpError):
        draw(eng, means.to(**TA(dtype)), S, mode_offset=3)
    assert eng.last_sample_kernel() == DENSE_PM

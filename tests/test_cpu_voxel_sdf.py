"""Host side of the voxel signed-distance field (SGPMP_COST_VOXEL_SDF): the numpy twin stoch_gpmp_amd/voxel_sdf.py against the
test-side oracle (tests/voxel_sdf_oracle.py: brute force, scipy, autograd) and hand values; the entry point in the header, the
binding and the built library; and the TEXT of the device functions (csrc/cost_device.h) compiled for the host as a stand-alone
program under AddressSanitizer + UBSan and held to the twin.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from stoch_gpmp_amd import voxel_sdf
from tests import voxel_sdf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SEED = 4            # of the configurations of the field tests (tests/test_gpu_voxel_sdf.py uses the same)


@pytest.mark.parametrize("name", list(O.small_volumes()) + list(O.mapping_volumes()))
def test_transform_equals_the_brute_force_exactly(name):
    occ, cell = {**O.small_volumes(), **O.mapping_volumes()}[name]
    got, ref = voxel_sdf.signed_distance_volume(occ, cell), O.brute_sdf(occ, cell)
    assert got.dtype == np.float64 and got.shape == occ.shape
    assert np.array_equal(got, ref), f"{name}: {int((got != ref).sum())} cells differ"
    assert np.isfinite(got).all()


def test_transform_caps_hand_values_and_argument_checks():
    sdv = voxel_sdf.signed_distance_volume
    assert sdv(np.zeros((1, 1, 1)), 0.5).tolist() == [[[1.5]]]                       # cap = cell (nx + ny + nz)
    assert sdv(np.ones((1, 1, 1)), 0.5).tolist() == [[[-1.5]]]
    assert np.array_equal(sdv(np.zeros((3, 4, 5)), 0.25), np.full((3, 4, 5), 3.0))
    assert np.array_equal(sdv(np.ones((3, 4, 5)), 0.25), np.full((3, 4, 5), -3.0))
    # one occupied cell in a line of five, cell 2: the zero level on the cell's faces -- along each axis in turn
    line = np.array([0., 0., 1., 0., 0.])
    for shape in ((1, 1, 5), (1, 5, 1), (5, 1, 1)):
        assert sdv(line.reshape(shape), 2.).ravel().tolist() == [3., 1., -1., 1., 3.], shape
    # the threshold: a cell is occupied when occ > threshold
    assert sdv(line.reshape(1, 1, 5) * 0.5, 2., threshold=0.5).ravel().tolist() == [14.] * 5     # nothing occupied: cap = 2 (5 + 1 + 1)
    # a single occupied cell in 3 x 4 x 5: every free cell's distance is to that cell; the space diagonal is sqrt(3) cells
    single, cell = O.small_volumes()["3x4x5 single cell"]
    s = sdv(single, cell)
    assert s[1, 2, 3] == -0.5 * cell and s[0, 1, 2] == (np.sqrt(3.) - 0.5) * cell and s[1, 2, 0] == 2.5 * cell
    assert s[2, 0, 0] == (np.sqrt(1. + 4. + 9.) - 0.5) * cell
    # the hollow box: the cavity's cells are free, one cell from the shell
    h = sdv(O.hollow_box(), 0.1)
    assert h[2, 2, 2] == 0.5 * 0.1 and h[1, 1, 1] == -0.5 * 0.1 and h[0, 0, 0] == (np.sqrt(3.) - 0.5) * 0.1
    for bad in (np.zeros((0, 3, 3)), np.zeros((3, 0, 3)), np.zeros((3, 3, 0)), np.zeros((5, 5)), np.zeros((1, 1, 513))):
        with pytest.raises(ValueError):
            sdv(bad, 0.1)
    for cell, thr in ((0., 0.), (-1., 0.), (0.1, float("nan"))):
        with pytest.raises(ValueError):
            sdv(np.zeros((2, 2, 2)), cell, thr)


def test_transform_equals_scipy_on_a_large_volume():
    pytest.importorskip("scipy.ndimage")
    occ, cell = O.large_volume()
    got, ref = voxel_sdf.signed_distance_volume(occ, cell), O.scipy_sdf(occ, cell)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} cells differ"
    assert float(np.abs(got).max()) > 10 * cell                      # distances of many cells occur
    # ... and scipy's form of the oracle is the brute force's on a volume both can do
    small, c2 = O.small_volumes()["9x10x11 random"]
    assert np.array_equal(O.scipy_sdf(small, c2), O.brute_sdf(small, c2))


def test_field_hand_values():
    # 2 x 2 x 3 volume, cell 2, offsets (1, 0, -1): cell centres at x = -1, 1, 3, y = 1, 3, z = 3, 5
    sdf = np.array([[[1., 2., 4.], [3., 6., 5.]], [[2., 4., 8.], [6., 12., 10.]]])        # [k][j][i]; the upper slice is the lower doubled
    cell, off = 2., (1., 0., -1.)
    f = lambda x, y, z, m=20.: [a.tolist() for a in voxel_sdf.field(sdf, cell, off, m, np.array([x, y, z]))]
    # cell centres: the cell's value; the slopes towards +x, +y, +z
    assert f(-1., 1., 3.) == [19., 1., [-0.5, -1., -0.5]]
    assert f(1., 3., 5.) == [8., 12., [1., 0., 0.]]             # top row and top slice: y and z clamp (no slope), x slope (10 - 12) / 2
    # on faces between cells
    assert f(0., 1., 3.) == [18.5, 1.5, [-0.5, -1.5, -0.75]]      # between i = 0 and 1: mean 1.5; dd/dy the mean of (3 - 1) / 2, (6 - 2) / 2
    assert f(-1., 2., 3.) == [18., 2., [-1., -1., -1.]]
    assert f(-1., 1., 4.) == [18.5, 1.5, [-0.75, -1.5, -0.5]]
    assert f(0., 2., 4.) == [15.5, 4.5, [-1.5, -2.25, -1.5]]      # a cell corner: the mean of eight cells
    # outside each of the six faces: clamp-to-edge, no slope across that face
    assert f(-9., 1., 3.) == [19., 1., [0., -1., -0.5]]
    assert f(99., 1., 3.) == [16., 4., [0., -0.5, -2.]]
    assert f(1., -7., 3.) == [18., 2., [-1., 0., -1.]]
    assert f(1., 50., 3.) == [14., 6., [0.5, 0., -3.]]
    assert f(1., 1., -9.) == [18., 2., [-1., -2., 0.]]
    assert f(1., 1., 77.) == [16., 4., [-2., -4., 0.]]
    assert f(-9., 50., 77.) == [14., 6., [0., 0., 0.]]
    # the hinge: inactive at d >= margin, value and gradient exactly zero
    assert f(1., 3., 5., 12.) == [0., 12., [0., 0., 0.]]
    assert f(1., 3., 5., 11.) == [0., 12., [0., 0., 0.]]
    assert f(1., 3., 5., 0.) == [0., 12., [0., 0., 0.]]
    # distance() is the middle value
    assert voxel_sdf.distance(sdf, cell, off, np.array([[0., 2., 4.], [99., 1., 3.]])).tolist() == [4.5, 4.]


def _arm_points(which, ni, B=200, seed=SEED):
    import torch
    chain, n, rng = O.CHAINS[which]
    q = O.draw_configs(which, B, seed)
    return q, O.link_points(torch.tensor(q), chain, ni, rng).numpy()


def test_field_gradient_matches_autograd_at_random_points():
    sc = O.arm_scene()
    tol = 1e-12 * max(1., sc["cell"] * sum(sc["sdf"].shape))
    q, pts = _arm_points("panda", 2)
    keep = O.regular(q, O.CHAINS["panda"][0], sc, 1e-6, 2)
    pts = pts[keep].reshape(-1, 3)
    h, d, g = voxel_sdf.field(sc["sdf"], sc["cell"], sc["origin"], sc["margin"], pts)
    ho, do, go = O.point_field_and_grad(sc["sdf"], pts, sc["cell"], sc["origin"], sc["margin"])
    assert (ho > 0).sum() >= 100 and (ho == 0).sum() >= 100 and (do < 0).any()
    assert np.abs(h - ho).max() <= tol and np.abs(d - do).max() <= tol and np.abs(g - go).max() <= tol
    assert float(np.abs(go).max()) > 0.5                               # (slopes of a distance field: about one)
    assert np.array_equal(g[ho == 0], np.zeros_like(g[ho == 0]))
    assert np.array_equal(voxel_sdf.distance(sc["sdf"], sc["cell"], sc["origin"], pts), d)
    # fp32 volume in, fp32 out
    h32, _, g32 = voxel_sdf.field(sc["sdf"].astype(np.float32), sc["cell"], sc["origin"], sc["margin"], pts)
    assert h32.dtype == np.float32 and g32.dtype == np.float32


@pytest.mark.parametrize("which", ["toy", "panda"])
@pytest.mark.parametrize("ni", [0, 2])
def test_the_seeded_configurations_meet_the_gpu_tests_conditions(which, ni):
    """What tests/test_gpu_voxel_sdf.py asks of its 200 configurations, on the fp64 oracle alone: at most 5 % lie within delta of a
    kink at both deltas (also after rounding q to fp32), points leave the volume on every side, some configurations are inactive
    everywhere and some are in collision."""
    sc = O.arm_scene()
    chain, n, rng = O.CHAINS[which]
    q, pts = _arm_points(which, ni)
    for delta, qq in ((1e-6, q), (1e-3, q), (1e-3, q.astype(np.float32).astype(np.float64))):
        left_out = int((~O.regular(qq, chain, sc, delta, ni, rng)).sum())
        assert left_out <= 0.05 * len(q), (delta, left_out)
    lo = np.array(sc["lower"])
    hi = lo + np.array(sc["sdf"].shape[::-1]) * sc["cell"]
    for a in range(3):
        assert (pts[..., a] < lo[a]).any() and (pts[..., a] > hi[a]).any(), a
    f, g, dmin, _ = O.config_field_and_grad(q, chain, sc, ni, rng)
    assert (f == 0).sum() >= 50 and (f > 0).sum() >= 50 and (dmin < 0).sum() >= 10
    assert np.array_equal(g[f == 0], np.zeros_like(g[f == 0]))


def test_field_nan_in_nan_out():
    sc = O.arm_scene()
    pts = np.array([[np.nan, 0., 0.3], [0., np.nan, 0.3], [0.1, 0.2, np.nan], [np.inf, 0., 0.3], [0., -np.inf, 0.3],
                    [0., 0.1, np.inf], [0.1, 0.2, 0.3]])
    h, d, g = voxel_sdf.field(sc["sdf"], sc["cell"], sc["origin"], 0.5, pts)
    assert np.isnan(h[:6]).all() and np.isnan(d[:6]).all() and np.isnan(g[:6]).all()
    assert np.isfinite(h[6]) and np.isfinite(g[6]).all()
    assert np.isnan(voxel_sdf.distance(sc["sdf"], sc["cell"], sc["origin"], pts)[:6]).all()


def test_header_binding_and_library_carry_the_entry_point():
    from stoch_gpmp_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgpmp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+sgpmp_voxel_sdf_build\s*\(\s*sgpmp_ctx\s*\*", code)
    assert re.search(r"\bSGPMP_COST_VOXEL_SDF\s*=\s*8\b", code)
    assert re.search(r"#define\s+SGPMP_ABI_VERSION\s+6\b", header)
    doc = header[header.index("voxel signed-distance field"):header.index("int sgpmp_voxel_sdf_build")]
    for word in ("clamp", "margin", "cell * (nx + ny + nz)", "SGPMP_EINVAL", "SGPMP_ESTATE", "NaN", "reserved = nz", "dt = oz",
                 "x first, then y, then z", "512"):
        assert word in doc, word
    lib = _lib.load()
    assert hasattr(lib, "sgpmp_voxel_sdf_build") and "sgpmp_voxel_sdf_build" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sgpmp_voxel_sdf_build"][1]) == 9         # the header's argument count
    assert _lib.COST_VOXEL_SDF == 8
    assert lib.sgpmp_abi_version() == _lib.ABI_VERSION == 6
    # argument checks come before any GPU work: a null context is refused
    assert lib.sgpmp_voxel_sdf_build(None, None, 4, 4, 4, 0.1, 0.0, None, None) == _lib.EINVAL
    assert "sgpmp_voxel_sdf_build" in _lib.last_error()
    # the classes and the twin are importable without a device
    from stoch_gpmp_amd.costs.fields import DistanceField
    from stoch_gpmp_amd.envs.voxel_map import VoxelDistanceField, VoxelMap
    assert callable(VoxelMap.distance_field) and issubclass(VoxelDistanceField, DistanceField)
    assert VoxelDistanceField.works_on_frames is True
    from stoch_gpmp_amd.engine import Engine
    assert callable(Engine.voxel_sdf_build)


# ------------------------------------------------------------------------------------------------ the device text on the host
@pytest.fixture(scope="module")
def host_field(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    d = tmp_path_factory.mktemp("host_voxel_sdf")
    src = open(os.path.join(ROOT, "stoch_gpmp_amd", "csrc", "cost_device.h")).read()
    a = src.index("// " + "-" * 82 + " voxel signed-distance field")
    text = src[a:src.index("// " + "-" * 82 + " signed-distance grid field", a)]
    assert "voxel_sdf_field(" in text and "voxel_sdf_distance(" in text
    (d / "voxel_sdf_funcs.inc").write_text(text)
    exe = str(d / "voxel_sdf_host")
    r = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(d), os.path.join(ROOT, "tests", "host_voxel_sdf", "main.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(sdf, pts, cell, off, margin, f64=True):
        nz, ny, nx = sdf.shape
        lines = [f"{int(f64)} {nz} {ny} {nx} {cell!r} {off[0]!r} {off[1]!r} {off[2]!r} {margin!r} {len(pts)}",
                 " ".join(repr(float(v)) for v in sdf.ravel())]
        lines += [f"{float(x)!r} {float(y)!r} {float(z)!r}" for x, y, z in pts]
        case = d / "case.txt"
        case.write_text("\n".join(lines) + "\n")
        res = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-3000:]      # (a sanitizer report fails the case)
        out = np.array([[float(v) for v in ln.split()] for ln in res.stdout.strip().splitlines()])
        return out[:, 0], out[:, 1], out[:, 2:]
    return run


def _special_points(sc):
    """Cell centres, points on cell-centre planes, cell corners, points outside the volume on every side and far out."""
    nz, ny, nx = sc["sdf"].shape
    cell, lo = sc["cell"], sc["lower"]
    c = lambda a, i: lo[a] + (i + 0.5) * cell
    pts = [(c(0, i), c(1, j), c(2, k)) for i in (0, 5, nx - 1) for j in (0, 7, ny - 1) for k in (0, 4, nz - 1)]       # centres
    pts += [(c(0, 4), c(1, 6) + 0.37 * cell, c(2, 3) + 0.2 * cell), (c(0, 9) + 0.61 * cell, c(1, 2), c(2, 8) - 0.1 * cell),
            (c(0, 2) + 0.3 * cell, c(1, 3) + 0.1 * cell, c(2, 5))]                                                       # on planes
    pts += [(c(0, i) + 0.5 * cell, c(1, j) + 0.5 * cell, c(2, k) + 0.5 * cell) for i, j, k in ((2, 2, 2), (9, 7, 4), (11, 12, 8))]
    pts += [(c(0, -5), c(1, 3) + 0.01, c(2, 4) + 0.02), (c(0, nx + 4), c(1, 8) + 0.03, c(2, 5)), (c(0, 6) + 0.02, c(1, -3), c(2, 2)),
            (c(0, 10) + 0.01, c(1, ny + 9), c(2, 6)), (c(0, 9), c(1, 6), c(2, -2)), (c(0, 9), c(1, 6), c(2, nz + 3)),
            (c(0, -2), c(1, -2), c(2, -2)), (c(0, nx + 1), c(1, ny + 1), c(2, nz + 1)), (-1e6, 0.3, 0.2), (0.2, 1e9, 0.2),
            (0.2, 0.1, -1e12)]                                                                                          # outside
    return np.array(pts)


def test_device_text_on_the_host_matches_the_twin(host_field):
    sc = O.arm_scene()
    sdf, cell, off = sc["sdf"], sc["cell"], sc["origin"]
    tol = 1e-12 * max(1., cell * sum(sdf.shape))
    _, pts = _arm_points("panda", 2, B=40)
    pts = np.concatenate((pts.reshape(-1, 3), _special_points(sc)))
    for margin in (O.MARGIN, 0.):
        h, d, g = host_field(sdf, pts, cell, off, margin)
        ht, dt, gt = voxel_sdf.field(sdf, cell, off, margin, pts)
        worst = max(np.abs(h - ht).max(), np.abs(d - dt).max(), np.abs(g - gt).max())
        print(f"    margin {margin}: worst |host text - twin| = {worst:.3e} (bound {tol:.1e}), {int((ht > 0).sum())} active of {len(pts)}")
        assert worst <= tol
        assert np.array_equal(g[ht == 0], np.zeros_like(g[ht == 0]))           # exactly zero where the hinge is inactive
        assert (ht > 0).any()
    # three different extents and three different offsets: an axis mix-up reads another cell (or past the volume: a sanitizer report)
    sdf2 = np.arange(60.).reshape(3, 4, 5) * 0.1 - 0.4
    pts2 = np.array([[100., 0.2, 0.1], [-100., 0.2, 0.1], [0.3, 100., 0.1], [0.3, -100., 0.1], [0.3, 0.2, 100.], [0.3, 0.2, -100.],
                     [0.33, 0.21, 0.4], [1.6, 0.9, 0.7]])
    h, d, g = host_field(sdf2, pts2, 0.5, (1., 2., 0.5), 9.)
    ht, dt, gt = voxel_sdf.field(sdf2, 0.5, (1., 2., 0.5), 9., pts2)
    assert np.abs(h - ht).max() <= 1e-12 and np.abs(d - dt).max() <= 1e-12 and np.abs(g - gt).max() <= 1e-12
    assert d[0] > d[1] + 0.39 and d[2] > d[3] + 1.4 and d[4] > d[5] + 3.9     # columns 4 / 0, rows 3 / 0, slices 2 / 0
    # fp32 instantiation: the twin in fp32 on the same volume, to fp32 rounding of two dozen flops
    h, d, g = host_field(sdf.astype(np.float32), pts[:300], cell, off, O.MARGIN, f64=False)
    ht, dt, gt = voxel_sdf.field(sdf.astype(np.float32), cell, off, O.MARGIN, pts[:300])
    assert np.abs(h - ht).max() <= 1e-5 and np.abs(g - gt).max() <= 1e-4


def test_device_text_on_the_host_keeps_a_nan(host_field):
    sc = O.arm_scene()
    pts = np.array([[np.nan, 0., 0.3], [0., np.nan, 0.3], [0.1, 0.2, np.nan], [np.inf, 0.1, 0.3], [0.1, -np.inf, 0.3],
                    [0.1, 0.2, np.inf], [np.nan, np.nan, np.nan], [0.1, 0.2, 0.3]])
    for f64 in (True, False):
        h, d, g = host_field(sc["sdf"], pts, sc["cell"], sc["origin"], 0.6, f64=f64)
        assert np.isnan(h[:7]).all() and np.isnan(d[:7]).all() and np.isnan(g[:7]).all()
        assert np.isfinite(h[7]) and np.isfinite(g[7]).all()

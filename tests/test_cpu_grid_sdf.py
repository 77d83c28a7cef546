"""Host side of the signed-distance grid field (SGPMP_COST_GRID_SDF): the numpy twin stoch_gpmp_amd/grid_sdf.py against the
test-side oracle (tests/grid_sdf_oracle.py: brute force, scipy, autograd) and hand values; the entry point in the header, the
binding and the built library; and the TEXT of the device functions (csrc/cost_device.h) compiled for the host under
AddressSanitizer + UBSan and held to the twin.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest

from stoch_gpmp_amd import grid_sdf
from tests import grid_sdf_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"


@pytest.mark.parametrize("name", list(O.small_maps()))
def test_transform_equals_the_brute_force_exactly(name):
    occ, cell = O.small_maps()[name]
    got, ref = grid_sdf.signed_distance_grid(occ, cell), O.brute_sdf(occ, cell)
    assert got.dtype == np.float64 and got.shape == occ.shape
    assert np.array_equal(got, ref), f"{name}: {int((got != ref).sum())} cells differ"
    assert np.isfinite(got).all()


def test_transform_caps_hand_values_and_argument_checks():
    assert grid_sdf.signed_distance_grid(np.zeros((1, 1)), 0.5).tolist() == [[1.0]]          # cap = cell (nx + ny)
    assert grid_sdf.signed_distance_grid(np.ones((1, 1)), 0.5).tolist() == [[-1.0]]
    assert grid_sdf.signed_distance_grid(np.zeros((3, 4)), 0.25).tolist() == [[1.75] * 4] * 3
    # one occupied cell in a row of five, cell 2: the zero level on the cell's edges
    row = np.array([[0., 0., 1., 0., 0.]])
    assert grid_sdf.signed_distance_grid(row, 2.).tolist() == [[3., 1., -1., 1., 3.]]
    # the threshold: a cell is occupied when occ > threshold
    assert grid_sdf.signed_distance_grid(row * 0.5, 2., threshold=0.5).tolist() == [[12.] * 5]   # nothing occupied: cap = 2 (5 + 1)
    # diagonal neighbours: sqrt(2) cells
    two = grid_sdf.signed_distance_grid(np.array([[0., 0.], [0., 1.]]), 1.)
    assert two[0, 0] == np.sqrt(2.) - 0.5 and two[0, 1] == 0.5 and two[1, 1] == -0.5
    for bad in (np.zeros((0, 3)), np.zeros((3, 0)), np.zeros(5), np.zeros((1, 4097))):
        with pytest.raises(ValueError):
            grid_sdf.signed_distance_grid(bad, 0.1)
    with pytest.raises(ValueError):
        grid_sdf.signed_distance_grid(np.zeros((2, 2)), 0.)


def test_transform_equals_scipy_on_a_large_map():
    pytest.importorskip("scipy.ndimage")
    occ, cell = O.large_map()
    got, ref = grid_sdf.signed_distance_grid(occ, cell), O.scipy_sdf(occ, cell)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} cells differ"
    assert float(np.abs(got).max()) > 20 * cell                      # distances of many cells occur
    # ... and scipy's form of the oracle is the brute force's on a map both can do
    small, c2 = O.small_maps()["20x24 box and disc"]
    assert np.array_equal(O.scipy_sdf(small, c2), O.brute_sdf(small, c2))


def test_field_hand_values():
    # 2 x 3 grid, cell 2, offsets (1, 0): cell centres at x = -1, 1, 3 and y = 1, 3
    sdf = np.array([[1., 2., 4.], [3., 6., 5.]])
    cell, off = 2., (1., 0.)
    f = lambda x, y, m=10.: [a.tolist() for a in grid_sdf.field(sdf, np.array([x, y]), cell, off, m)]
    assert f(-1., 1.) == [9., 1., [-0.5, -1.]]                 # a cell centre: the value of the cell; the slope towards +x, +y
    assert f(1., 3.) == [4., 6., [0.5, 0.]]                    # top row: y clamps (no slope in y), x slope (5 - 6) / 2
    assert f(0., 2.) == [7., 3., [-1., -1.5]]                  # a cell corner: the mean of four cells
    assert f(2., 1.) == [7., 3., [-1., -1.25]]                 # an edge midpoint
    # outside on each side: clamp-to-edge, no slope across the border
    assert f(-9., 1.) == [9., 1., [0., -1.]]
    assert f(99., 1.) == [6., 4., [0., -0.5]]
    assert f(1., -7.) == [8., 2., [-1., 0.]]
    assert f(1., 50.) == [4., 6., [0.5, 0.]]
    assert f(-9., 50.) == [7., 3., [0., 0.]]
    # the hinge: inactive at d >= margin, value and gradient exactly zero
    assert f(1., 3., 6.) == [0., 6., [0., 0.]]
    assert f(1., 3., 5.) == [0., 6., [0., 0.]]
    assert f(1., 3., 0.) == [0., 6., [0., 0.]]
    # x is clamped by the x extent (3 cells), y by the y extent (2): a point far out in x reads column 2
    assert f(1000., 1.)[1] == 4.


def test_field_gradient_matches_autograd_at_random_points():
    occ, cell, off = O.box_disc_map()
    sdf = grid_sdf.signed_distance_grid(occ, cell)
    margin = O.MARGIN
    pts = O.draw_points(sdf, cell, off, margin, 256, seed=3, tol=1e-3)
    h, d, g = grid_sdf.field(sdf, pts, cell, off, margin)
    ho, do, go = O.field_and_grad(sdf, pts, cell, off, margin)
    cap = cell * (sdf.shape[0] + sdf.shape[1])
    tol = 1e-12 * max(1., cap)
    assert (ho > 0).sum() >= 256 // 3 and (ho == 0).any()
    assert np.abs(h - ho).max() <= tol and np.abs(d - do).max() <= tol and np.abs(g - go).max() <= tol
    assert np.array_equal(g[ho == 0], np.zeros_like(g[ho == 0]))
    # fp32 grid in, fp32 out
    h32, _, g32 = grid_sdf.field(sdf.astype(np.float32), pts, cell, off, margin)
    assert h32.dtype == np.float32 and g32.dtype == np.float32


def test_field_nan_in_nan_out():
    occ, cell, off = O.box_disc_map()
    sdf = grid_sdf.signed_distance_grid(occ, cell)
    pts = np.array([[np.nan, 0.], [0., np.nan], [np.inf, 0.], [0., -np.inf], [0.1, 0.2]])
    h, d, g = grid_sdf.field(sdf, pts, cell, off, 0.5)
    assert np.isnan(h[:4]).all() and np.isnan(d[:4]).all() and np.isnan(g[:4]).all()
    assert np.isfinite(h[4]) and np.isfinite(g[4]).all()


def test_header_binding_and_library_carry_the_entry_point():
    from stoch_gpmp_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgpmp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+sgpmp_grid_sdf_build\s*\(\s*sgpmp_ctx\s*\*", code)
    assert re.search(r"\bSGPMP_COST_GRID_SDF\s*=\s*7\b", code)
    assert re.search(r"#define\s+SGPMP_FLAG_GRID_DISTANCE\s+64\b", code)
    assert re.search(r"#define\s+SGPMP_ABI_VERSION\s+6\b", header)
    for word in ("clamp", "margin", "cell * (nx + ny)", "SGPMP_EINVAL", "SGPMP_ESTATE", "NaN"):
        assert word in header[header.index("signed-distance grid field"):header.index("int sgpmp_grid_sdf_build")], word
    lib = _lib.load()
    assert hasattr(lib, "sgpmp_grid_sdf_build") and "sgpmp_grid_sdf_build" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sgpmp_grid_sdf_build"][1]) == 8          # the header's argument count
    assert _lib.COST_GRID_SDF == 7 and _lib.FLAG_GRID_DISTANCE == 64
    assert lib.sgpmp_abi_version() == _lib.ABI_VERSION == 6
    # argument checks come before any GPU work: a null context is refused
    assert lib.sgpmp_grid_sdf_build(None, None, 4, 4, 0.1, 0.0, None, None) == _lib.EINVAL
    assert "sgpmp_grid_sdf_build" in _lib.last_error()
    # the classes and the twin are importable without a device
    from stoch_gpmp_amd.envs.obst_map import GridDistanceField, ObstacleMap
    assert callable(ObstacleMap.distance_field) and GridDistanceField.needs_fk_chain is False


# ------------------------------------------------------------------------------------------------ the device text on the host
@pytest.fixture(scope="module")
def host_field(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    d = tmp_path_factory.mktemp("host_grid_sdf")
    src = open(os.path.join(ROOT, "stoch_gpmp_amd", "csrc", "cost_device.h")).read()
    a = src.index("// " + "-" * 82 + " signed-distance grid field")
    text = src[a:src.index("// " + "-" * 82 + " generic FK (LDS)", a)]
    assert "grid_sdf_field(" in text and "grid_sdf_distance(" in text
    (d / "grid_sdf_funcs.inc").write_text(text)
    exe = str(d / "grid_sdf_host")
    r = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(d), os.path.join(ROOT, "tests", "host_grid_sdf", "main.cpp"),
                        "-o", exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(sdf, pts, cell, off, margin, f64=True):
        ny, nx = sdf.shape
        lines = [f"{int(f64)} {ny} {nx} {cell!r} {off[0]!r} {off[1]!r} {margin!r} {len(pts)}",
                 " ".join(repr(float(v)) for v in sdf.ravel())]
        lines += [f"{float(x)!r} {float(y)!r}" for x, y in pts]
        case = d / "case.txt"
        case.write_text("\n".join(lines) + "\n")
        res = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and not res.stderr.strip(), res.stderr[-3000:]      # (a sanitizer report fails the case)
        out = np.array([[float(v) for v in ln.split()] for ln in res.stdout.strip().splitlines()])
        return out[:, 0], out[:, 1], out[:, 2:]
    return run


def _special_points(sdf, cell, off):
    """Cell centres, points exactly on cell-centre lines, cell corners, points outside the map on every side."""
    ny, nx = sdf.shape
    cx = lambda i: (i + 0.5 - off[0]) * cell
    cy = lambda j: (j + 0.5 - off[1]) * cell
    pts = [(cx(i), cy(j)) for i in (0, 3, nx - 1) for j in (0, 7, ny - 1)]                     # centres
    pts += [(cx(4), cy(6) + 0.37 * cell), (cx(9) + 0.61 * cell, cy(2)), (cx(11), cy(12) - 0.2 * cell)]   # on centre lines
    pts += [(cx(i) + 0.5 * cell, cy(j) + 0.5 * cell) for i, j in ((2, 2), (10, 7), (14, 12))]   # corners
    pts += [(cx(-5), cy(3) + 0.1), (cx(nx + 4), cy(8) + 0.03), (cx(6) + 0.02, cy(-3)), (cx(12) + 0.01, cy(ny + 9)),
            (cx(-2), cy(-2)), (cx(nx + 1), cy(ny + 1)), (-1e6, 0.3), (0.2, 1e9)]                # outside
    return np.array(pts)


def test_device_text_on_the_host_matches_the_twin(host_field):
    occ, cell, off = O.box_disc_map()
    sdf = grid_sdf.signed_distance_grid(occ, cell)
    cap = cell * (sdf.shape[0] + sdf.shape[1])
    tol = 1e-12 * max(1., cap)
    for margin in (O.MARGIN, 0.):
        pts = np.concatenate((O.draw_points(sdf, cell, off, O.MARGIN, 256, seed=3, tol=1e-3), _special_points(sdf, cell, off)))
        h, d, g = host_field(sdf, pts, cell, off, margin)
        ht, dt, gt = grid_sdf.field(sdf, pts, cell, off, margin)
        worst = max(np.abs(h - ht).max(), np.abs(d - dt).max(), np.abs(g - gt).max())
        print(f"    margin {margin}: worst |host text - twin| = {worst:.3e} (bound {tol:.1e}), {int((ht > 0).sum())} active of {len(pts)}")
        assert worst <= tol
        assert np.array_equal(g[ht == 0], np.zeros_like(g[ht == 0]))           # exactly zero where the hinge is inactive
    # a non-square map with other offsets: x clamps by the x extent
    sdf2 = np.arange(15.).reshape(3, 5) * 0.1 - 0.4
    pts = np.array([[100., 0.2], [-100., 0.2], [0.3, 100.], [0.3, -100.], [0.33, 0.21]])
    h, d, g = host_field(sdf2, pts, 0.5, (1., 2.), 0.7)
    ht, dt, gt = grid_sdf.field(sdf2, pts, 0.5, (1., 2.), 0.7)
    assert np.abs(h - ht).max() <= 1e-12 and np.abs(d - dt).max() <= 1e-12 and np.abs(g - gt).max() <= 1e-12
    assert d[0] > d[1] + 0.39                                   # column 4 on the right, column 0 on the left
    # fp32 instantiation: the twin in fp32 on the same grid, to fp32 rounding of a dozen flops
    pts = O.draw_points(sdf, cell, off, 0.6, 64, seed=5, tol=1e-2)
    h, d, g = host_field(sdf.astype(np.float32), pts, cell, off, 0.6, f64=False)
    ht, dt, gt = grid_sdf.field(sdf.astype(np.float32), pts, cell, off, 0.6)
    assert np.abs(h - ht).max() <= 1e-5 * max(1., cap) and np.abs(g - gt).max() <= 1e-4


def test_device_text_on_the_host_keeps_a_nan(host_field):
    occ, cell, off = O.box_disc_map()
    sdf = grid_sdf.signed_distance_grid(occ, cell)
    pts = np.array([[np.nan, 0.], [0., np.nan], [np.inf, 0.1], [0.1, -np.inf], [np.nan, np.nan], [0.1, 0.2]])
    for f64 in (True, False):
        h, d, g = host_field(sdf, pts, cell, off, 0.6, f64=f64)
        assert np.isnan(h[:5]).all() and np.isnan(d[:5]).all() and np.isnan(g[:5]).all()
        assert np.isfinite(h[5]) and np.isfinite(g[5]).all()

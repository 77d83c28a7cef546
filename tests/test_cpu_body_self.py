"""Host side of the body's self-collision term (SGPMP_COST_BODY_SELF): the numpy twin stoch_gpmp_amd/body_self.py against the
test-side oracle (tests/body_self_oracle.py: torch fp64, autograd through the FK) and the oracle's gradient against central
differences; BodySpheres.pair_rows; the entry point in the header, the binding and the built library; the conditions the GPU tests
place on their seeded inputs; and the TEXT of the device functions (csrc/body_self_device.h) compiled for the host as a stand-alone
program under AddressSanitizer + UBSan and held to the twin.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle.fk import fk_all_links
from stoch_gpmp_amd import body_sdf, body_self
from stoch_gpmp_amd.robots.body import BodySpheres
from tests import body_self_oracle as SO
from tests import voxel_sdf_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
CASES = ["M=2", "along_links", "M=64", "behind a fixed joint", "link 0 against the last"]


def chain_of(which):
    return VO.CHAINS[which][0]


def reach(chain):
    return sum(float(np.linalg.norm(j[3])) for j in chain)


@pytest.mark.parametrize("which", ["toy", "panda"])
def test_twin_equals_the_oracle(which):
    chain = chain_of(which)
    q = VO.draw_configs(which, 130, SO.SEED)
    tol = 1e-12
    for name, (body, rows, margin) in SO.cases(which).items():
        f, g, smin, gs = body_self.config_field(margin, q, chain, body, rows)
        fo, go, so, gso, s_all, D = SO.config_field_and_grad(q, chain, body, rows, margin)
        gap = SO.argmin_gap(s_all) > 1e-9
        errs = (np.abs(f - fo).max(), np.abs(g - go).max(), np.abs(smin - so).max(), np.abs(gs - gso)[gap].max())
        print(f"    {which} {name}: |twin - oracle| value {errs[0]:.2e} grad {errs[1]:.2e} clearance {errs[2]:.2e} its grad {errs[3]:.2e}")
        assert errs[0] <= tol and errs[2] <= tol and errs[1] <= tol * reach(chain) and errs[3] <= tol * reach(chain)
        # the frames path: clearances and the field on the oracle's frames, in summation order
        frames = fk_all_links(torch.as_tensor(q), chain)
        assert np.abs(body_self.clearance(frames.numpy(), body, rows) - s_all).max() <= tol
        ff = body_self.field(margin, frames.numpy(), body, rows)[0]
        assert np.abs(ff - SO.frames_field(frames, body, rows, margin).numpy()).max() <= tol
        assert np.abs(SO.frames_clearance(frames, body, rows).numpy() - s_all).max() <= tol
        if name == "behind a fixed joint":
            assert np.array_equal(g, np.zeros_like(g)) and np.array_equal(gs, np.zeros_like(gs)) and (f > 0).all()
        else:
            assert (fo > 0).any() and (go != 0).any()


@pytest.mark.parametrize("which", ["toy", "panda"])
def test_oracle_gradient_equals_central_differences(which):
    """Steps of h = 1e-6 in fp64.  Per counted pair the rounding error of the quotient is about 2e-16 / 2h = 1e-10, and the
    truncation error is h^2 / 6 times a third derivative, which for |p_i - p_j| is of the order reach^3 / D^2: 3e-10 at the
    D = 0.02 of a typical active pair.  Hence 1e-9 per counted pair, and 1e-8 for the query, which is one pair at any D >= 5e-3.
    The seeded inputs keep every pair 1e-5 m from the hinge's kink (test_seeded_inputs_meet_the_gpu_tests_conditions), several
    times the move of a centre under a step (h times the reach), so no pair changes sides."""
    chain, n = chain_of(which), VO.CHAINS[which][1]
    q = VO.draw_configs(which, 130, SO.SEED)[:24]
    for name, (body, rows, margin) in SO.cases(which).items():
        _, g, _, gs, s, _ = SO.config_field_and_grad(q, chain, body, rows, margin)
        h = 1e-6
        num, nums = np.zeros_like(g), np.zeros_like(gs)
        for k in range(n):
            dq = np.zeros_like(q)
            dq[:, k] = h
            fp, _, sp, _, _, _ = SO.config_field_and_grad(q + dq, chain, body, rows, margin)
            fm, _, sm, _, _, _ = SO.config_field_and_grad(q - dq, chain, body, rows, margin)
            num[:, k], nums[:, k] = (fp - fm) / (2 * h), (sp - sm) / (2 * h)
        gap = SO.argmin_gap(s) > 1e-4
        bound = 1e-9 * max(1, s.shape[1])
        err = (np.abs(g - num).max(), np.abs(gs - nums)[gap].max())
        print(f"    {which} {name}: |autograd - central differences| {err[0]:.2e}, of the query {err[1]:.2e} (bound {bound:.1e})")
        assert err[0] <= bound and err[1] <= 1e-8


def test_oracle_defines_the_two_singular_points():
    """A placeholder chain with exactly representable positions: a revolute joint about z at the origin, then a fixed offset of
    (0.25, 0, 0).  D exactly 0 (both spheres at the joint's origin, whatever q) and, at q = 0, D exactly at margin + r_i + r_j."""
    chain = [("j0", "revolute", (0., 0., 0.), (0., 0., 0.)), ("j1", "fixed", (0., 0., 0.), (0.25, 0., 0.))]
    q = np.array([[0.3], [1.1]])
    zero = BodySpheres([0, 1], [(0., 0., 0.), (0., 0., 0.)], [0.125, 0.25])
    f, g, smin, gs, s, D = SO.config_field_and_grad(q, chain, zero, [2, 0], 0.5)
    ft, gt, st, gst = body_self.config_field(0.5, q, chain, zero, [2, 0])
    for a, b in ((f, ft), (g, gt), (smin, st), (gs, gst)):
        assert np.array_equal(a, b)
    assert np.array_equal(f, [0.875, 0.875]) and np.array_equal(g, np.zeros((2, 1))) and np.array_equal(D, np.zeros((2, 1)))
    assert np.array_equal(smin, [-0.375, -0.375]) and np.array_equal(gs, np.zeros((2, 1)))
    edge = BodySpheres([0, 2], [(0., 0., 0.), (0., 0., 0.)], [0.0625, 0.0625])           # D = 0.25 = 0.125 + 2 * 0.0625
    q = np.zeros((1, 1))
    f, g, _, _, _, D = SO.config_field_and_grad(q, chain, edge, [2, 0], 0.125)
    ft, gt, _, _ = body_self.config_field(0.125, q, chain, edge, [2, 0])
    assert np.array_equal(D, [[0.25]]) and np.array_equal(f, [0.]) and np.array_equal(g, np.zeros((1, 1)))
    assert np.array_equal(ft, f) and np.array_equal(gt, g)


def test_pair_rows_on_the_panda_chain():
    chain = chain_of("panda")
    body = BodySpheres.along_links(chain, SO.SPACING, SO.RADIUS)
    links = list(body.links)
    rows = body.pair_rows()
    assert rows == SO.rows_by_gap(links, 2) == body_self.pair_rows(links, 2)
    pairs = body_self.pair_list(rows)
    assert len(pairs) == 119 and all(links[j] - links[i] >= 2 for i, j in pairs)
    assert all((i, j) in pairs for i in range(len(links)) for j in range(i + 1, len(links)) if links[j] - links[i] >= 2)
    i, j = SO.pairs_of(rows)
    assert list(zip(i.tolist(), j.tolist())) == pairs                        # the same summation order
    assert body.pair_rows(min_link_gap=1) == SO.rows_by_gap(links, 1) and body.pair_rows(min_link_gap=10) == SO.rows_by_gap(links, 10)
    # the ignore list drops link pairs, in either order
    less = body.pair_rows(ignore=[(4, 2), (0, 10)])
    got = body_self.pair_list(less)
    assert set(got) == {(a, b) for a, b in pairs if (links[a], links[b]) not in ((2, 4), (0, 10))} and len(got) < len(pairs)
    assert less == body_self.pair_rows(links, 2, ignore=[(2, 4), (10, 0)])
    # an empty result raises
    for bad in (lambda: body.pair_rows(min_link_gap=11), lambda: body.pair_rows(min_link_gap=0),
                lambda: BodySpheres([0, 2], [(0, 0, 0)] * 2, [0.1] * 2).pair_rows(ignore=[(0, 2)]),
                lambda: BodySpheres([3, 3], [(0, 0, 0), (0.1, 0, 0)], [0.1] * 2).pair_rows(min_link_gap=1),
                lambda: body_self.pair_rows([0, 1], 2)):
        with pytest.raises(ValueError):
            bad()
    for rows in (rows, less):
        assert all(0 <= r < 2 ** 64 and r >> len(links) == 0 and r & ((2 << k) - 1) == 0 for k, r in enumerate(rows))


def test_nan_in_nan_out():
    chain = chain_of("toy")
    body, rows, margin = SO.cases("toy")["along_links"]
    q = VO.draw_configs("toy", 4, SO.SEED)
    q[1, 0] = np.nan
    q[2, 1] = np.inf
    out = body_self.config_field(margin, q, chain, body, rows)
    ref = SO.config_field_and_grad(q, chain, body, rows, margin)[:4]
    for arr, want in zip(out, ref):
        assert np.isnan(arr[1]).all() and np.isnan(arr[2]).all() and np.isfinite(arr[0]).all() and np.isfinite(arr[3]).all()
        assert np.isnan(want[1]).all() and np.isnan(want[2]).all() and np.isfinite(want[0]).all()
    # a NaN behind every counted sphere changes nothing: the last joint of the toy chain moves the last link only
    base, brow, _ = SO.cases("toy")["M=2"]
    q2 = VO.draw_configs("toy", 2, SO.SEED)
    assert base.links[-1] == 3
    q2[1, 2] = np.nan                  # joint 2 is in front of link 3: the pair is lost
    f, g, _, _ = body_self.config_field(0.3, q2, chain, base, brow)
    assert np.isfinite(f[0]) and np.isnan(f[1]) and np.isnan(g[1]).all()


def test_header_binding_and_library_carry_the_entry_point():
    from stoch_gpmp_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgpmp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+sgpmp_set_body_pairs\s*\(\s*sgpmp_ctx\s*\*\s*\w*\s*,\s*const\s+uint64_t\s*\*", code)
    assert re.search(r"\bSGPMP_COST_BODY_SELF\s*=\s*10\b", code) and re.search(r"\bSGPMP_COST_BODY_SDF\s*=\s*9\b", code)
    assert re.search(r"#define\s+SGPMP_ABI_VERSION\s+6\b", header)
    doc = header[header.index("body self-collision: sphere pairs"):header.index("int sgpmp_set_body_pairs")]
    for word in ("only bits j > i are read", "SGPMP_EINVAL", "SGPMP_ESTATE", "sgpmp_set_body and sgpmp_set_fk clear the pairs", "NaN",
                 "margin + r_i + r_j", "num_interpolate must be 0", "i ascending, then j ascending", "FIRST arg-min", "exactly 0",
                 "D_ij = 0", "one link", "no counted pair", "SGPMP_FLAG_GRID_DISTANCE", "sgpmp_dense_cost", "sgpmp_validate",
                 "constant address space", "Synchronous"):
        assert word.lower() in doc.lower(), word
    lib = _lib.load()
    assert hasattr(lib, "sgpmp_set_body_pairs") and len(_lib.SIGNATURES["sgpmp_set_body_pairs"][1]) == 3
    assert _lib.COST_BODY_SELF == 10
    assert lib.sgpmp_abi_version() == _lib.ABI_VERSION == 6
    # argument checks come before any GPU work: a null context is refused
    assert lib.sgpmp_set_body_pairs(None, None, 3) == _lib.EINVAL
    assert "sgpmp_set_body_pairs" in _lib.last_error()
    from stoch_gpmp_amd.costs.fields import BodySelfDistanceField, DistanceField
    from stoch_gpmp_amd.engine import Engine
    assert issubclass(BodySelfDistanceField, DistanceField) and callable(Engine.set_body_pairs)
    assert BodySelfDistanceField.works_on_frames is True and "dense_cost=" in BodySelfDistanceField.__doc__
    body = BodySpheres.along_links(chain_of("panda"), SO.SPACING, SO.RADIUS)
    fld = BodySelfDistanceField(body, 0.05)
    dsc = fld.descriptor(0.1)
    assert dsc["kind"] == 10 and dsc["body"] is body and list(dsc["body_pairs"]) == body.pair_rows() and dsc["sigma2"] == 0.05
    assert fld.num_pairs == 119 and fld.descriptor(0.1, distance=True)["flags"] == _lib.FLAG_GRID_DISTANCE
    assert BodySelfDistanceField(body, 0.05, ignore=[(0, 10)]).num_pairs < 119
    for bad in (lambda: BodySelfDistanceField(body, -0.1), lambda: BodySelfDistanceField(body, 0.1, pairs=[1, 2]),
                lambda: BodySelfDistanceField(BodySpheres([0], [(0, 0, 0)], [0.1]), 0.1)):
        with pytest.raises(ValueError):
            bad()


def test_seeded_inputs_meet_the_gpu_tests_conditions():
    """Every counted pair of every random case of tests/test_gpu_body_self.py: |margin - s_ij| >= 1e-5 m and D_ij >= 1e-3 m."""
    for which in ("toy", "panda"):
        q = VO.draw_configs(which, 130, SO.SEED)
        for name, (body, rows, margin) in SO.cases(which).items():
            f, _, smin, _, s, D = SO.config_field_and_grad(q, chain_of(which), body, rows, margin)
            kink, dmin = SO.conditions(s, D, margin)
            print(f"    {which} {name}: {s.shape[1]} pairs, min |margin - s| {kink:.2e}, min D {dmin:.2e}, active {100 * (f > 0).mean():.0f} %, "
                  f"overlapping {100 * (smin < 0).mean():.0f} %")
            assert kink >= 1e-5 and dmin >= 1e-3
            assert (f > 0).any()


# ------------------------------------------------------------------------------------------------ the device text on the host
@pytest.fixture(scope="module")
def host_self(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    d = tmp_path_factory.mktemp("host_body_self")
    csrc = os.path.join(ROOT, "stoch_gpmp_amd", "csrc")
    exe = str(d / "body_self_host")
    r = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", csrc,
                        os.path.join(ROOT, "tests", "host_body_self", "main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(margin, chain, body, rows, q, f64=True):
        lines = [f"{int(f64)} {margin!r}", str(len(chain))]
        k = 0
        for _, kind, rpy, xyz in chain:
            rev = kind == "revolute"
            lines.append(" ".join(repr(float(v)) for v in list(body_sdf._rpy(rpy).ravel()) + list(xyz)) + f" {int(rev)} {k if rev else -1}")
            k += rev
        lines.append(str(len(body)))
        lines += [f"{l} " + " ".join(repr(float(v)) for v in row) for l, row in zip(body.links, body.table())]
        lines.append(" ".join(str(int(r)) for r in rows))
        lines.append(f"{k} {len(q)}")
        lines += [" ".join(repr(float(v)) for v in row) for row in q]
        case = d / "case.txt"
        case.write_text("\n".join(lines) + "\n")
        res = subprocess.run([exe, str(case)], capture_output=True, text=True, timeout=600)
        assert res.returncode == 0 and not res.stderr.strip(), (res.returncode, res.stderr[-3000:])   # (a sanitizer report fails the case)
        out = np.array([[float(v) for v in ln.split()] for ln in res.stdout.strip().splitlines()])
        return out[:, 0], out[:, 1:1 + k], out[:, 1 + k], out[:, 2 + k:2 + 2 * k], out[:, 2 + 2 * k]
    return run


@pytest.mark.parametrize("which", ["toy", "panda"])
def test_device_text_on_the_host_matches_the_twin(host_self, which):
    chain = chain_of(which)
    q = VO.draw_configs(which, 130, SO.SEED)[:48]
    tol = 1e-12
    for name, (body, rows, margin) in SO.cases(which).items():
        for mg in (margin, 0.):
            f, g, s, gs, ff = host_self(mg, chain, body, rows, q)
            ft, gt, st, gst = body_self.config_field(mg, q, chain, body, rows)
            worst = max(np.abs(f - ft).max(), np.abs(s - st).max(), np.abs(ff - ft).max())
            worst_g = max(np.abs(g - gt).max(), np.abs(gs - gst).max())
            print(f"    {which} {name}, margin {mg}: worst |host text - twin| value {worst:.2e} (bound {tol:.1e}), gradient {worst_g:.2e} "
                  f"(bound {tol * reach(chain):.1e}); {int((ft > 0).sum())} active of {len(q)}")
            assert worst <= tol and worst_g <= tol * reach(chain)
        if name == "behind a fixed joint":
            assert np.array_equal(g, np.zeros_like(g)) and np.array_equal(gs, np.zeros_like(gs))
    # the other compiled-in chain length, 7 joints with n_dof 7: the Panda without its three fixed hand joints (the driver holds
    # the compiled-in form to the generic one bit for bit)
    if which == "panda":
        arm = chain[:7]
        body7 = BodySpheres.along_links(arm, SO.SPACING, SO.RADIUS)
        rows7 = SO.rows_by_gap(body7.links, 2)
        f, g, s, gs, ff = host_self(0.15, arm, body7, rows7, q)
        ft, gt, st, gst = body_self.config_field(0.15, q, arm, body7, rows7)
        assert max(np.abs(f - ft).max(), np.abs(s - st).max(), np.abs(ff - ft).max()) <= tol and (np.abs(gt) > 0).any()
        assert max(np.abs(g - gt).max(), np.abs(gs - gst).max()) <= tol * reach(arm)
    # the last sphere of a full table in a pair (bit 63), and a row with bits at and below the diagonal (not read)
    body, rows, margin = SO.cases(which)["M=64"]
    top = [0] * 64
    top[0] = 1 << 63
    assert body.links[0] != body.links[63]
    f, g, s, gs, ff = host_self(0.5, chain, body, top, q[:8])
    ft, gt, st, gst = body_self.config_field(0.5, q[:8], chain, body, top)
    assert max(np.abs(f - ft).max(), np.abs(s - st).max(), np.abs(ff - ft).max()) <= tol and (ft > 0).any()
    low = [r | ((2 << k) - 1) for k, r in enumerate(rows)]
    assert np.array_equal(host_self(margin, chain, body, low, q[:8])[0], host_self(margin, chain, body, rows, q[:8])[0])
    # fp32 instantiation against the fp64 twin, to fp32 rounding of the walk (the project's 3e-4 of tests/test_gpu_body_sdf.py)
    body, rows, margin = SO.cases(which)["along_links"]
    f, g, s, gs, ff = host_self(margin, chain, body, rows, q, f64=False)
    ft, gt, st, gst = body_self.config_field(margin, q, chain, body, rows)
    assert np.abs(f - ft).max() <= 3e-4 * max(1., np.abs(ft).max()) and np.abs(s - st).max() <= 3e-4
    assert np.abs(g - gt).max() <= 3e-4 * max(1., np.abs(gt).max())


def test_device_text_on_the_host_keeps_a_nan_and_the_singular_points(host_self):
    chain = chain_of("toy")
    body, rows, margin = SO.cases("toy")["along_links"]
    q = VO.draw_configs("toy", 4, SO.SEED)
    q[1, 0] = np.nan
    q[2, 1] = np.inf
    for f64 in (True, False):
        f, g, s, gs, ff = host_self(margin, chain, body, rows, q, f64=f64)
        for arr in (f, g, s, gs, ff):
            assert np.isnan(arr[1]).all() and np.isnan(arr[2]).all() and np.isfinite(arr[0]).all() and np.isfinite(arr[3]).all()
    # D = 0 and D exactly at the hinge's edge, on exactly representable positions
    ph = [("j0", "revolute", (0., 0., 0.), (0., 0., 0.)), ("j1", "fixed", (0., 0., 0.), (0.25, 0., 0.))]
    qq = np.array([[0.3], [1.1]])
    for f64 in (True, False):
        f, g, s, gs, ff = host_self(0.5, ph, BodySpheres([0, 1], [(0., 0., 0.)] * 2, [0.125, 0.25]), [2, 0], qq, f64=f64)
        assert np.array_equal(f, [0.875] * 2) and np.array_equal(ff, f) and np.array_equal(g, np.zeros((2, 1)))
        assert np.array_equal(s, [-0.375] * 2) and np.array_equal(gs, np.zeros((2, 1)))
    f, g, s, gs, ff = host_self(0.125, ph, BodySpheres([0, 2], [(0., 0., 0.)] * 2, [0.0625, 0.0625]), [2, 0], np.zeros((1, 1)))
    assert np.array_equal(f, [0.]) and np.array_equal(ff, f) and np.array_equal(g, np.zeros((1, 1))) and np.array_equal(s, [0.125])

"""Host side of the body collision spheres on the voxel field (SGPMP_COST_BODY_SDF): the numpy twin stoch_gpmp_amd/body_sdf.py
against the test-side oracle (tests/body_sdf_oracle.py: torch fp64, autograd through the FK); BodySpheres.along_links; the entry
point in the header, the binding and the built library; and the TEXT of the device functions (csrc/body_device.h) compiled for the
host as a stand-alone program under AddressSanitizer + UBSan and held to the twin.  No GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle.fk import fk_all_links
from stoch_gpmp_amd import body_sdf, voxel_sdf
from stoch_gpmp_amd.robots.body import BodySpheres
from tests import body_sdf_oracle as BO
from tests import voxel_sdf_oracle as VO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
SEED = 3            # of the configurations of the field tests (tests/test_gpu_body_sdf.py uses the same)
SPACING, RADIUS = 0.12, 0.06
PANDA_LINKS = [0, 0, 0, 1, 2, 2, 2, 3, 4, 4, 4, 4, 5, 6, 7, 8, 9, 10]
TOY_LINKS = [0, 0, 1, 1, 2, 2, 2, 2, 3, 3, 3, 4]


def chain_of(which):
    return VO.CHAINS[which][0]


def body_of(which):
    return BodySpheres.along_links(chain_of(which), SPACING, RADIUS)


def reach(chain):
    return sum(float(np.linalg.norm(j[3])) for j in chain)


def test_along_links_reproduces_the_documented_tables():
    p, t = body_of("panda"), body_of("toy")
    assert len(p) == 18 and list(p.links) == PANDA_LINKS
    assert len(t) == 12 and list(t.links) == TOY_LINKS
    assert set(p.radii) == {RADIUS}
    # joint 4's offset (-0.0825, 0.384, 0) in four steps on link 4; the last link's sphere at its origin
    assert p.centers[8] == (0., 0., 0.) and np.allclose(p.centers[11], (-0.0825 * 0.75, 0.384 * 0.75, 0.))
    assert p.centers[-1] == (0., 0., 0.) and p.links[-1] == len(chain_of("panda"))
    # no two consecutive spheres of a link further apart than the spacing
    for body, chain in ((p, chain_of("panda")), (t, chain_of("toy"))):
        for l, j in enumerate(chain):
            k = list(body.links).count(l)
            assert np.linalg.norm(j[3]) / k <= SPACING + 1e-12


def test_body_spheres_sorts_stably_and_validates():
    b = BodySpheres([2, 0, 2, 1], [(1, 0, 0), (2, 0, 0), (3, 0, 0), (4, 0, 0)], [0.1, 0.2, 0.3, 0.4])
    assert b.links == (0, 1, 2, 2) and b.radii == (0.2, 0.4, 0.1, 0.3) and b.centers[2] == (1., 0., 0.)
    assert b.table()[3] == [3., 0., 0., 0.3]
    assert b == BodySpheres([0, 1, 2, 2], [(2, 0, 0), (4, 0, 0), (1, 0, 0), (3, 0, 0)], [0.2, 0.4, 0.1, 0.3])
    assert b != BodySpheres([0, 1, 2, 2], [(2, 0, 0), (4, 0, 0), (1, 0, 0), (3, 0, 0)], [0.2, 0.4, 0.1, 0.31])
    for bad in (lambda: BodySpheres([], [], []), lambda: BodySpheres([0] * 65, [(0, 0, 0)] * 65, [0.] * 65),
                lambda: BodySpheres([0], [(0, 0, 0)], [-0.1]), lambda: BodySpheres([0], [(0, 0, float("nan"))], [0.1]),
                lambda: BodySpheres([0], [(0, 0, 0)], [float("inf")]), lambda: BodySpheres([-1], [(0, 0, 0)], [0.1]),
                lambda: BodySpheres([0, 1], [(0, 0, 0)], [0.1, 0.1]), lambda: BodySpheres.along_links(chain_of("toy"), 0., 0.1)):
        with pytest.raises(ValueError):
            bad()


@pytest.mark.parametrize("which", ["toy", "panda"])
def test_twin_equals_the_oracle(which):
    sc, chain, body = VO.arm_scene(), chain_of(which), body_of(which)
    q = VO.draw_configs(which, 256, SEED)
    cap = sc["cell"] * sum(sc["sdf"].shape)
    tol = 1e-12 * max(1., cap)
    f, g, smin, gs = body_sdf.config_field(sc["sdf"], sc["cell"], sc["origin"], sc["margin"], q, chain, body)
    fo, go, so, gso, s_all = BO.config_field_and_grad(q, chain, body, sc)
    reg = BO.regular(q, chain, body, sc, 1e-6)
    gap = BO.argmin_gap(s_all) > 1e-9
    errs = (np.abs(f - fo).max(), np.abs(g - go)[reg].max(), np.abs(smin - so).max(), np.abs(gs - gso)[reg & gap].max())
    print(f"    {which}: |twin - oracle| value {errs[0]:.2e} grad {errs[1]:.2e} clearance {errs[2]:.2e} its grad {errs[3]:.2e} "
          f"(bounds {tol:.1e}, {tol * reach(chain):.1e}); {int(reg.sum())} of {len(q)} regular")
    assert errs[0] <= tol and errs[2] <= tol
    assert errs[1] <= tol * reach(chain) and errs[3] <= tol * reach(chain)
    assert (fo > 0).any() and (go[reg] != 0).any()
    # the frames path: points, clearances and the field on the oracle's frames
    frames = fk_all_links(torch.as_tensor(q), chain)
    assert np.abs(body_sdf.body_points(frames.numpy(), body) - BO.frames_points(frames, body).numpy()).max() <= 1e-14
    assert np.abs(body_sdf.clearance(sc["sdf"], sc["cell"], sc["origin"], frames.numpy(), body) - s_all).max() <= tol
    ff = body_sdf.field(sc["sdf"], sc["cell"], sc["origin"], sc["margin"], frames.numpy(), body)[0]
    assert np.abs(ff - BO.frames_field(frames, body, sc).numpy()).max() <= tol
    # the twin's own frames are the oracle's
    assert np.abs(body_sdf.link_frames(q, chain)[0] - frames.numpy()).max() <= 1e-14


@pytest.mark.parametrize("which", ["toy", "panda"])
def test_zero_offset_zero_radius_body_is_the_voxel_field_at_the_link_origins(which):
    sc, chain = VO.arm_scene(), chain_of(which)
    L = len(chain) + 1
    body = BodySpheres(range(L), [(0., 0., 0.)] * L, [0.] * L)
    q = VO.draw_configs(which, 64, SEED)
    frames = fk_all_links(torch.as_tensor(q), chain).numpy()
    f = body_sdf.field(sc["sdf"], sc["cell"], sc["origin"], sc["margin"], frames, body)[0]
    h = voxel_sdf.field(sc["sdf"], sc["cell"], sc["origin"], sc["margin"], frames[..., :3, 3])[0]
    assert np.abs(f - h.sum(-1)).max() <= 1e-12 and (f > 0).any()
    fo = VO.config_field_and_grad(q, chain, sc)[0]
    assert np.abs(f - fo).max() <= 1e-12


def test_nan_in_nan_out():
    sc, chain, body = VO.arm_scene(), chain_of("toy"), body_of("toy")
    q = VO.draw_configs("toy", 4, SEED)
    q[1, 2] = np.nan          # the last revolute joint: the spheres behind it are lost, the value and every entry with them
    q[2, 0] = np.inf
    f, g, smin, gs = body_sdf.config_field(sc["sdf"], sc["cell"], sc["origin"], sc["margin"], q, chain, body)
    for arr in (f, g, smin, gs):
        assert np.isnan(arr[1]).all() and np.isnan(arr[2]).all() and np.isfinite(arr[0]).all() and np.isfinite(arr[3]).all()
    frames = body_sdf.link_frames(q, chain)[0]
    assert np.isnan(body_sdf.clearance(sc["sdf"], sc["cell"], sc["origin"], frames, body)[1]).any()
    # a body on link 0 alone does not depend on q at all
    base = BodySpheres([0], [(0.1, 0., 0.2)], [0.05])
    f0, g0, _, _ = body_sdf.config_field(sc["sdf"], sc["cell"], sc["origin"], 0.6, q, chain, base)
    assert np.isfinite(f0).all() and (f0 > 0).all() and np.array_equal(g0, np.zeros_like(g0))


def test_header_binding_and_library_carry_the_entry_point():
    from stoch_gpmp_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgpmp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+sgpmp_set_body\s*\(\s*sgpmp_ctx\s*\*", code)
    assert re.search(r"\bSGPMP_COST_BODY_SDF\s*=\s*9\b", code) and re.search(r"#define\s+SGPMP_MAX_BODY\s+64\b", code)
    assert re.search(r"#define\s+SGPMP_ABI_VERSION\s+6\b", header)
    doc = header[header.index("body collision spheres on the voxel field"):header.index("int sgpmp_set_body")]
    for word in ("non-decreasing", "SGPMP_EINVAL", "SGPMP_ESTATE", "sgpmp_set_fk clears the body", "NaN", "margin + r_m",
                 "num_interpolate must be 0", "table order", "first", "SGPMP_FLAG_GRID_DISTANCE", "sgpmp_dense_cost"):
        assert word.lower() in doc.lower(), word
    lib = _lib.load()
    assert hasattr(lib, "sgpmp_set_body") and len(_lib.SIGNATURES["sgpmp_set_body"][1]) == 4
    assert _lib.COST_BODY_SDF == 9 and _lib.MAX_BODY == 64
    assert lib.sgpmp_abi_version() == _lib.ABI_VERSION == 6
    # argument checks come before any GPU work: a null context is refused
    assert lib.sgpmp_set_body(None, None, None, 3) == _lib.EINVAL
    assert "sgpmp_set_body" in _lib.last_error()
    from stoch_gpmp_amd.costs.fields import DistanceField
    from stoch_gpmp_amd.engine import Engine
    from stoch_gpmp_amd.envs.voxel_map import BodyDistanceField, VoxelMap
    assert callable(VoxelMap.body_field) and issubclass(BodyDistanceField, DistanceField) and callable(Engine.set_body)
    assert BodyDistanceField.works_on_frames is True


def test_seeded_inputs_meet_the_gpu_tests_conditions():
    sc, chain, body = VO.arm_scene(), chain_of("panda"), body_of("panda")
    q = VO.draw_configs("panda", 256, SEED)
    f, _, smin, _, _ = BO.config_field_and_grad(q, chain, body, sc)
    out6 = 1. - BO.regular(q, chain, body, sc, 1e-6).mean()
    out3 = 1. - BO.regular(q, chain, body, sc, 1e-3).mean()
    toy3 = 1. - BO.regular(VO.draw_configs("toy", 256, SEED), chain_of("toy"), body_of("toy"), sc, 1e-3).mean()
    print(f"    panda: outside regular {100 * out6:.1f} % at 1e-6, {100 * out3:.1f} % at 1e-3 (toy {100 * toy3:.1f} %); "
          f"active {100 * (f > 0).mean():.0f} %, penetrating {100 * (smin < 0).mean():.0f} %, clear by > 0.05 "
          f"{100 * (smin > 0.05).mean():.0f} %")
    assert out6 == 0. and out3 <= 0.10 and toy3 <= 0.10
    assert (f > 0).mean() >= 0.25 and (smin < 0).sum() >= 5 and (smin > 0.05).sum() >= 5


# ------------------------------------------------------------------------------------------------ the device text on the host
@pytest.fixture(scope="module")
def host_body(tmp_path_factory):
    if not os.path.exists(CLANG):
        pytest.skip("no clang++")
    d = tmp_path_factory.mktemp("host_body_sdf")
    csrc = os.path.join(ROOT, "stoch_gpmp_amd", "csrc")
    src = open(os.path.join(csrc, "cost_device.h")).read()
    a = src.index("// " + "-" * 82 + " voxel signed-distance field")
    text = src[a:src.index("// " + "-" * 82 + " signed-distance grid field", a)]
    assert "voxel_sdf_field(" in text and "voxel_sdf_distance(" in text
    (d / "voxel_sdf_funcs.inc").write_text(text)
    exe = str(d / "body_sdf_host")
    r = subprocess.run([CLANG, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=undefined", "-I", str(d), "-I", csrc,
                        os.path.join(ROOT, "tests", "host_body_sdf", "main.cpp"), "-o", exe],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(sc, margin, chain, body, q, f64=True):
        sdf = sc["sdf"]
        nz, ny, nx = sdf.shape
        off = sc["origin"]
        lines = [f"{int(f64)} {nz} {ny} {nx} {sc['cell']!r} {off[0]!r} {off[1]!r} {off[2]!r} {margin!r}",
                 " ".join(repr(float(v)) for v in sdf.ravel()), str(len(chain))]
        k = 0
        for _, kind, rpy, xyz in chain:
            rev = kind == "revolute"
            lines.append(" ".join(repr(float(v)) for v in list(body_sdf._rpy(rpy).ravel()) + list(xyz)) + f" {int(rev)} {k if rev else -1}")
            k += rev
        lines.append(str(len(body)))
        lines += [f"{l} " + " ".join(repr(float(v)) for v in row) for l, row in zip(body.links, body.table())]
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
def test_device_text_on_the_host_matches_the_twin(host_body, which):
    sc, chain, body = VO.arm_scene(), chain_of(which), body_of(which)
    q = VO.draw_configs(which, 96, SEED)
    tol = 1e-12 * max(1., sc["cell"] * sum(sc["sdf"].shape))
    for margin in (VO.MARGIN, 0.):
        f, g, s, gs, ff = host_body(sc, margin, chain, body, q)
        ft, gt, st, gst = body_sdf.config_field(sc["sdf"], sc["cell"], sc["origin"], margin, q, chain, body)
        worst = max(np.abs(f - ft).max(), np.abs(s - st).max(), np.abs(ff - ft).max())
        worst_g = max(np.abs(g - gt).max(), np.abs(gs - gst).max())
        print(f"    {which}, margin {margin}: worst |host text - twin| value {worst:.2e} (bound {tol:.1e}), gradient {worst_g:.2e} "
              f"(bound {tol * reach(chain):.1e}); {int((ft > 0).sum())} active of {len(q)}")
        assert worst <= tol and worst_g <= tol * reach(chain)
        assert (ft > 0).any()
    # a body of the largest size, spheres on every link, radii that differ; one sphere on the last link only; link 0 only
    rng = np.random.default_rng(5)
    L = len(chain) + 1
    big = BodySpheres(rng.integers(0, L, 64), rng.uniform(-0.1, 0.1, (64, 3)), rng.uniform(0., 0.12, 64))
    for b in (big, BodySpheres([L - 1], [(0.02, -0.01, 0.03)], [0.07]), BodySpheres([0, 0], [(0.1, 0., 0.2), (0.3, 0.1, 0.3)], [0.05, 0.2])):
        f, g, s, gs, ff = host_body(sc, 0.2, chain, b, q[:24])
        ft, gt, st, gst = body_sdf.config_field(sc["sdf"], sc["cell"], sc["origin"], 0.2, q[:24], chain, b)
        assert max(np.abs(f - ft).max(), np.abs(s - st).max(), np.abs(ff - ft).max()) <= tol
        assert max(np.abs(g - gt).max(), np.abs(gs - gst).max()) <= tol * reach(chain)
        if b.links[-1] == 0:
            assert np.array_equal(g, np.zeros_like(g)) and np.array_equal(gs, np.zeros_like(gs)) and (f > 0).all()
    # fp32 instantiation: the twin in fp32 on the same volume, to fp32 rounding of the walk
    sc32 = dict(sc, sdf=sc["sdf"].astype(np.float32))
    f, g, s, gs, ff = host_body(sc32, VO.MARGIN, chain, body, q[:48], f64=False)
    ft, gt, st, gst = body_sdf.config_field(sc["sdf"], sc["cell"], sc["origin"], VO.MARGIN, q[:48], chain, body)
    reg = BO.regular(q[:48], chain, body, sc, 1e-3)
    assert np.abs(f - ft)[reg].max() <= 3e-4 * max(1., np.abs(ft).max()) and np.abs(s - st).max() <= 3e-4
    assert np.abs(g - gt)[reg].max() <= 3e-4 * max(1., np.abs(gt).max())


def test_device_text_on_the_host_keeps_a_nan(host_body):
    sc, chain, body = VO.arm_scene(), chain_of("toy"), body_of("toy")
    q = VO.draw_configs("toy", 4, SEED)
    q[1, 2] = np.nan
    q[2, 0] = np.inf
    for f64 in (True, False):
        scx = sc if f64 else dict(sc, sdf=sc["sdf"].astype(np.float32))
        f, g, s, gs, ff = host_body(scx, 0.6, chain, body, q, f64=f64)
        for arr in (f, g, s, gs, ff):
            assert np.isnan(arr[1]).all() and np.isnan(arr[2]).all() and np.isfinite(arr[0]).all() and np.isfinite(arr[3]).all()

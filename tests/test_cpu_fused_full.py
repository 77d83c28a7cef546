"""The choice between fused_step_kernel's generic instantiation and the one with the four-term program compiled in
(csrc/step_plan.hip: fused_full_variant), on the CPU."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC, CLANGXX = "/opt/rocm/bin/hipcc", "/opt/rocm/lib/llvm/bin/clang++"


def test_fused_full_variant_rule_under_sanitizers(tmp_path):
    """tests/host_asan/fused_full_table.cpp: the REAL csrc/step_plan.hip compiled host-only with -fsanitize=address,undefined and a
    stand-alone program that walks the rule over every launch mode x program, and plan_step over the cases that must and must
    not take the compiled-in program (end-effector term, missing term, GP term without start prior, armed partials, store-free
    steps, shapes off the grid, the small-step launch, run-time chains, the fused_generic switch)."""
    if not os.path.exists(HIPCC) or not os.path.exists(CLANGXX):
        pytest.skip("no ROCm clang")
    d = os.path.join(ROOT, "tests", "host_asan")
    csrc = os.path.join(ROOT, "stoch_gpmp_amd", "csrc")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1"]
    host = [HIPCC, "--cuda-host-only", "-std=c++17", f"-I{csrc}", f"-I{os.path.join(ROOT, 'include')}", f"-I{d}", "-Wno-unused-value"] + san
    objs = []
    for src in (os.path.join(csrc, "step_plan.hip"), os.path.join(d, "fused_full_table.cpp")):
        obj = str(tmp_path / (os.path.basename(src) + ".o"))
        r = subprocess.run(host + ["-c", src, "-o", obj], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        objs.append(obj)
    exe = str(tmp_path / "fused_full_table")
    r = subprocess.run([CLANGXX] + san + objs + ["-o", exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    env = {k: v for k, v in os.environ.items() if not k.startswith("SGPMP_")}
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    p = subprocess.run([exe], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "FUSED_FULL_OK" in p.stdout, (p.stdout[-1000:], p.stderr[-4000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-4000:]


def test_compiled_in_instantiations_are_audited_like_the_generic_kernels():
    """tools/audit_asm_loads.py walks the six fused_step_kernel instantiations with the program compiled in (3 field types x
    {without, with the softmax partials}) as it walks the others -- no hand-placed load's destination touched before its wait,
    no scratch -- and counts them on a line of their own."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "audit_asm_loads.py")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert re.search(r"^6 instantiations with the cost program compiled in audited, [1-9]\d* hand-placed loads, 0 offending", r.stdout, re.M), r.stdout
    assert "0 kernels with scratch" in r.stdout, r.stdout

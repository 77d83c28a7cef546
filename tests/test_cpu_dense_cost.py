"""Host side of the continuous-time cost (sgpmp_dense_cost): the numpy helpers of stoch_gpmp_amd/dense.py against hand values,
and the two entry points in the header, the binding and the built library.  No GPU."""
import os
import re

import numpy as np
import pytest

from stoch_gpmp_amd import dense

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_inserted_indices():
    assert dense.inserted_indices(2, 0).tolist() == []
    assert dense.inserted_indices(5, 0).tolist() == []
    assert dense.inserted_indices(2, 1).tolist() == [1]
    assert dense.inserted_indices(3, 2).tolist() == [1, 2, 4, 5]
    assert dense.inserted_indices(4, 3).tolist() == [1, 2, 3, 5, 6, 7, 9, 10, 11]
    for T, k in ((2, 31), (66, 3), (7, 4)):
        ins = dense.inserted_indices(T, k)
        support = np.arange(T) * (k + 1)
        assert len(ins) == (T - 1) * k and not set(ins) & set(support)
        assert sorted(set(ins) | set(support)) == list(range(dense.fine_length(T, k)))     # every fine state exactly once
    with pytest.raises(ValueError):
        dense.inserted_indices(1, 2)


def test_limit_penalty_hand_values():
    # one dof, three fine states (q, v): q_lo - q = 0.5 at the first, q - q_hi = 0.25 at the last, |v| - v_max = 1 and 2
    fine = np.array([[[-1.5, 0.0], [0.0, -3.0], [1.25, 4.0]]])
    lim = (([-1.0], [1.0]), [2.0])
    assert dense.limit_penalty(fine, *lim, sigma_limit=1.0).tolist() == [0.25 + 0.0625 + 1.0 + 4.0]
    assert dense.limit_penalty(fine, *lim, sigma_limit=0.5).tolist() == [4 * 5.3125]
    # one side alone, the velocity alone, nothing
    assert dense.limit_penalty(fine, ([-1.0], None), None, 1.0).tolist() == [0.25]
    assert dense.limit_penalty(fine, (None, [1.0]), None, 1.0).tolist() == [0.0625]
    assert dense.limit_penalty(fine, None, [2.0], 1.0).tolist() == [5.0]
    assert dense.limit_penalty(fine).tolist() == [0.0]
    assert dense.limit_penalty(fine, (None, None), None).tolist() == [0.0]
    # inside every limit: exactly 0; leading dimensions are kept; per-dof limits
    two = np.zeros((2, 3, 4, 4))
    two[1, 2, 0] = [0.5, -2.0, 0.1, 0.3]                                 # q = (0.5, -2), v = (0.1, 0.3)
    out = dense.limit_penalty(two, ([-1.0, -1.5], [1.0, 1.5]), [0.2, 0.2], 0.1)
    assert out.shape == (2, 3) and out[0].tolist() == [0.0, 0.0, 0.0]
    assert out[1, :2].tolist() == [0.0, 0.0] and abs(out[1, 2] - (0.25 + 0.01) / 0.01) < 1e-12
    for bad in (None, 0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            dense.limit_penalty(fine, *lim, sigma_limit=bad)


def test_header_binding_and_library_carry_the_entry_points():
    from stoch_gpmp_amd import _lib
    header = open(os.path.join(ROOT, "include", "sgpmp.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+sgpmp_dense_cost\s*\(\s*sgpmp_ctx\s*\*", code)
    assert re.search(r"\bconst\s+char\s*\*\s*sgpmp_last_dense_kernel\s*\(\s*void\s*\)", code)
    assert re.search(r"#define\s+SGPMP_ABI_VERSION\s+6\b", header)
    lib = _lib.load()
    for name in ("sgpmp_dense_cost", "sgpmp_last_dense_kernel"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["sgpmp_dense_cost"][1]) == 16            # the header's argument count
    assert lib.sgpmp_abi_version() == _lib.ABI_VERSION == 6
    name = lib.sgpmp_last_dense_kernel()                                 # "" until this thread launches one
    assert name == b"" or name.startswith(b"dense_cost_kernel")
    # argument checks come before any GPU work: a null context is refused
    assert lib.sgpmp_dense_cost(None, None, 1, 1, 0.05, None, 0, 1.0, None, None, None, 0.0, 0, None, None, None) == _lib.EINVAL
    assert "sgpmp_dense_cost" in _lib.last_error()

"""The report of the sampler launch (include/sgpmp.h: sgpmp_last_sample_kernel) on the CPU: declared, bound, and empty on a
thread that has not launched a sampler.  What it reports after a launch is tests/test_gpu_sampler.py's business."""
import ctypes
import os
import re
import threading

from stoch_gpmp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_the_sampler_report_under_the_same_abi():
    src = open(os.path.join(ROOT, "include", "sgpmp.h")).read()
    assert re.search(r"^const char\* sgpmp_last_sample_kernel\(void\);", src, flags=re.M)
    assert re.search(r"#define SGPMP_ABI_VERSION 6\b", src) and _lib.ABI_VERSION == 6     # a query, not a new ABI
    assert _lib.SIGNATURES["sgpmp_last_sample_kernel"] == (ctypes.c_char_p, [])
    # an older build of this ABI may lack it and still load; the set that test_cpu_gpmp_dense.py holds to one member stays as it is
    assert "sgpmp_last_sample_kernel" in _lib.ADDED_LATER_UNDER_THIS_ABI
    assert "sgpmp_last_sample_kernel" not in _lib.ADDED_UNDER_THIS_ABI


def test_engine_has_the_query():
    from stoch_gpmp_amd.engine import Engine
    assert callable(Engine.last_sample_kernel)


def test_report_is_empty_on_a_thread_that_launched_nothing():
    """The record is per thread (like sgpmp_last_gpmp_kernel's): a thread started here has enqueued no sampler, whatever the
    tests that ran before this one did on theirs."""
    lib = _lib.load()
    assert hasattr(lib, "sgpmp_last_sample_kernel"), "the library of this tree must export it"
    got = []
    t = threading.Thread(target=lambda: got.append(lib.sgpmp_last_sample_kernel()))
    t.start()
    t.join()
    assert got == [b""]

"""CPU: the host side of the ragged launch path (tests/test_ragged_launch_gpu.py has the solves) -- the diagnostic
entry point flamed_den_lens_path is declared, exported, bound and documented, the knob ragged_launch exists, and the
contract of flamed_den_solve_lens in the header says what the launch path does with the padding rows.  No GPU call."""
import ctypes
import os

from _common import PKG

ROOT = os.path.dirname(PKG)


def test_lens_path_declared_bound_and_documented():
    from flamed import _native as nat
    diag = open(os.path.join(ROOT, "include", "flamed_diag.h")).read()
    hip_part = diag.split("---- libflamed_hip.so diagnostics ----")[1]
    assert "FLAMED_API int flamed_den_lens_path(flamed_den_t h, int* path);" in hip_part
    assert "flamed_den_lens_path" in nat.HIP_DIAG_SIGNATURES and "flamed_den_lens_path" not in nat.SIGNATURES
    assert "flamed_den_lens_path" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    L = nat.lib()
    assert L.flamed_den_lens_path.argtypes == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    path = ctypes.c_int(7)
    assert L.flamed_den_lens_path(None, ctypes.byref(path)) == 1001
    assert b"flamed_den_lens_path" in L.flamed_last_error()
    h = ctypes.c_void_p()
    assert L.flamed_den_create(256, 1024, 4, 31, 256, 1, ctypes.byref(h)) == 0
    try:
        assert L.flamed_den_lens_path(h, None) == 1001
        assert L.flamed_den_lens_path(h, ctypes.byref(path)) == 0 and path.value == -1  # no _lens solve yet
    finally:
        assert L.flamed_den_destroy(h) == 0
    from flamed.models.synthesizer.prob_generator import DenoiserHIP
    assert callable(DenoiserHIP.lens_path)


def test_ragged_launch_knob():
    from flamed import _native as nat
    L = nat.lib()
    assert L.flamed_tune(b"ragged_launc", 1) == 1001  # (a boolean knob: any non-zero value is 1)
    assert L.flamed_tune(b"ragged_launch", 0) == 0
    assert L.flamed_tune(b"ragged_launch", 1) == 0  # the default
    h = ctypes.c_void_p()
    assert L.flamed_den_create(256, 1024, 4, 31, 256, 1, ctypes.byref(h)) == 0
    try:
        assert L.flamed_den_tune(h, b"ragged_launch", 0) == 0
    finally:
        assert L.flamed_den_destroy(h) == 0
    hdr = open(os.path.join(ROOT, "include", "flamed_hip.h")).read()
    assert '"ragged_launch"' in hdr


def test_header_contract_of_solve_lens():
    hdr = " ".join(open(os.path.join(ROOT, "include", "flamed_hip.h")).read().split())
    i = hdr.index("Exact lengths: the same solves for a padded ragged batch")
    text = hdr[i:hdr.index("FLAMED_API int flamed_den_solve_lens(", i)].replace(" * ", " ")
    assert "never influence a valid row and are never written" in text
    assert "they may be read" in text
    assert "ws as for (B, T)" in text
    assert "neither read nor written" not in text

"""CPU: szn_augment_affine_u8 is declared in include/szn.h with szn_augment_u8's parameter list, exported by libszn_hip.so and bound in
_lib.SIGNATURES with the matching signature; SZN_AUGA_NPARAM is 20 on both sides; bad arguments are refused on the host before anything
touches a device; the Python surface carries the new names."""
import ctypes
import inspect
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NAME = "szn_augment_affine_u8"


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "szn.h")).read(), flags=re.S)


def _header_params(name):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_entry_and_its_record_size():
    params = _header_params(NAME)
    assert params == ["int B", "int Hm", "int Wm", "const uint8_t* rgb_hwc", "const int64_t* label", "const int32_t* params",
                      "const double* mean_bgr", "int Ho", "int Wo", "float* out_nchw", "int64_t* out_label", "szn_stream_t stream"]
    assert params == _header_params("szn_augment_u8")
    assert re.search(r"#define\s+SZN_AUGA_NPARAM\s+20\b", _header()) and re.search(r"#define\s+SZN_AUG_NPARAM\s+9\b", _header())
    # the two identities are stated where the contract is
    text = " ".join(open(os.path.join(ROOT, "include", "szn.h")).read().split())
    assert "identity colour" in text and "axis-aligned" in text and "(a + 2k) >> 1 == (a >> 1) + k" in text


def test_binding_matches_the_header():
    from zeroshotsemanticsegmentation_amd import _lib as L
    assert L.AUGA_NPARAM == 20 and L.AUG_NPARAM == 9
    res, args = L.SIGNATURES[NAME]
    assert res is L._I and len(args) == len(_header_params(NAME))
    want = [L._I if p.startswith("int ") else (ctypes.POINTER(ctypes.c_double) if p.startswith("const double*") else L._P)
            for p in _header_params(NAME)]
    assert args == want and L.SIGNATURES[NAME] == L.SIGNATURES["szn_augment_u8"]


def test_library_exports_the_entry_and_refuses_bad_arguments():
    import __graft_entry__ as g
    from zeroshotsemanticsegmentation_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        g.build()
    assert hasattr(ctypes.CDLL(L.LIB_PATH), NAME)
    lib = L.load()
    assert lib.szn_version() >= 116
    # refused on the host, before anything touches a device (the buffer only stands for non-NULL, 16-byte aligned pointers)
    raw = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p((ctypes.addressof(raw) + 15) & ~15)
    mean = (ctypes.c_double * 3)(1.0, 2.0, 3.0)
    fn = getattr(lib, NAME)
    good = [1, 4, 4, p, p, p, mean, 4, 4, p, p, None]
    for i in (3, 4, 5, 6, 9, 10):
        bad = list(good)
        bad[i] = None
        assert fn(*bad) != 0 and b"required" in lib.szn_last_error()
    for i, v in ((0, 0), (0, -1), (1, 0), (2, -3), (7, 0), (8, 0), (8, -4), (0, 65536)):
        bad = list(good)
        bad[i] = v
        assert fn(*bad) != 0 and b"augment_affine_u8" in lib.szn_last_error()


def test_python_surface():
    from zeroshotsemanticsegmentation_amd import datasets, utils
    names = list(inspect.signature(datasets.Augment.__init__).parameters)
    assert names == ["self", "crop", "scale", "flip", "seed", "rotate", "jitter"]
    sig = inspect.signature(datasets.Augment.__init__).parameters
    assert sig["rotate"].default == 0.0 and sig["jitter"].default is None
    assert list(inspect.signature(utils.augment_affine_to_device).parameters) == list(inspect.signature(utils.augment_to_device).parameters)

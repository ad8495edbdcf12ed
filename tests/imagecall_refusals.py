"""What the five composite calls of the image front end (detection, then K24's refinement: csrc/abi_imagecall.hpp) refuse alike, for the
refusal tests of test_chess_host.py, test_boardorder_host.py and test_tags_host.py: every field of the refinement options on its own,
calls with two things wrong (which refusal comes first), and the corner count.  No call here needs a handle or a device."""
import ctypes as C

import numpy as np

from camlasercalibratool_amd import _capi

FIND_FORMS = ("clc_find_chessboard", "clc_find_chessboard_device", "clc_find_chessboard_gpu")
TAG_FORMS = ("clc_tag_grid", "clc_tag_grid_device")

# every field of clc_subpix_options out of its range, the others at clc_subpix_options_default(3)
SUBPIX_FAULTS = [dict(win_x=16), dict(win_y=0), dict(max_iter=0), dict(max_iter=101), dict(eps=float("nan")), dict(eps=-0.1), dict(reserved=1)]
REFINEMENT_TEXT = "%s: the refinement options are not valid (clc_corner_subpix)"

_CODES = np.array([0x1234], np.uint64)
_IMG = np.zeros((1, 16, 16), np.uint8)
_OUT = np.zeros(4096, np.float64)  # (nothing reads or writes the arrays of a refused call)


def subpix(**kw):
    o = _capi.SubpixOptions(3, 3, -1, -1, 30, 0, 0.1)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def chess(**kw):
    o = _capi.ChessOptions(500, 3, 250, 256, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def call(L, name, copt=None, oopt=None, sopt=None, width=16, height=16, pitch=16, n=1, cols=5, rows=4, arrays=True):
    """One call of a composite form with a NULL handle -> (code, the message)."""
    ref = lambda o: None if o is None else C.byref(o)
    img, out = _IMG.ctypes.data_as(C.c_void_p), (_OUT.ctypes.data_as(C.c_void_p) if arrays else None)
    if name in FIND_FORMS:
        code = getattr(L, name)(None, ref(copt), ref(oopt), ref(sopt), img, width, height, pitch, n, cols, rows, out, out, None)
    else:
        assert oopt is None
        fam = _capi.TagFamilyC(4, 2, 1, 0, _CODES.ctypes.data)
        code = getattr(L, name)(None, C.byref(fam), None, ref(copt), ref(sopt), img, width, height, pitch, n, cols, rows, out, out, out, out,
                                None, None, None, None)
    return code, L.clc_last_error().decode()


# Calls with two things wrong.  The find forms: a detection option and the geometry, the geometry and the order options, the order
# options and max_per_image < cols x rows, the refinement options and a NULL array.  The tag forms have no order options: the grid's
# shape stands in their place, and their third pair is the detection's geometry and the refinement options.
_BAD_ORDER = dict(oopt=_capi.ChessOrderOptions(0.7, 0, 0))
PAIRS = {
    "find": [dict(copt=chess(threshold=0), width=0), dict(width=0, **_BAD_ORDER), dict(copt=chess(max_per_image=19), **_BAD_ORDER),
             dict(sopt=subpix(win_x=16), arrays=False)],
    "tag": [dict(copt=chess(threshold=0), width=0), dict(width=0, cols=0), dict(pitch=15, sopt=subpix(win_x=16)),
            dict(sopt=subpix(win_x=16), arrays=False)],
}
# What the product library of commit a8ac6b6 (the parent of the change that gave the family one check per rule) answers to PAIRS,
# row by row, after the caller's name: recorded by running this table on that build.
PAIR_TEXTS = {
    "find": ["threshold must be >= 1", "width and height must be >= 1", "tol must be in (0, 0.5]", "bad argument"],
    "tag": ["threshold must be >= 1", "cols and rows must be >= 1 and cols x rows <= 1024", "pitch must be >= width",
            "the refinement options are not valid (clc_corner_subpix)"],
}


def check_composite_refusals(L, name):
    """The rows every composite form gets: see the module's docstring."""
    kind = "find" if name in FIND_FORMS else "tag"
    for fault in SUBPIX_FAULTS:
        code, msg = call(L, name, sopt=subpix(**fault))
        assert code == -1 and msg == REFINEMENT_TEXT % name, (name, fault, code, msg)
    for kw, text in zip(PAIRS[kind], PAIR_TEXTS[kind]):
        code, msg = call(L, name, **kw)
        assert code == -1 and msg == "%s: %s" % (name, text), (name, kw, code, msg)
    # 2^31 corners of 16 x 16 images: refused by name among the argument checks where a refinement is asked for, and only there
    big = dict(copt=chess(max_per_image=1024), cols=32, rows=32, n=2 ** 21 if kind == "find" else 2 ** 19)
    code, msg = call(L, name, sopt=subpix(), **big)
    assert code == -1 and msg == name + ": too many corners", (name, code, msg)
    code, msg = call(L, name, **big)
    assert code == -1 and msg == name + ": bad argument", (name, code, msg)  # nothing wrong but the NULL handle
    code, msg = call(L, name, sopt=subpix(), **dict(big, n=big["n"] - 1))
    assert code == -1 and msg == name + ": bad argument", (name, code, msg)  # 2^31 - cols x rows (x 4) corners: allowed
    # the refinement options are looked at before the count, the count before a NULL array (tag forms) or the NULL handle
    assert call(L, name, sopt=subpix(win_x=16), **big)[1] == REFINEMENT_TEXT % name
    if kind == "tag":
        assert call(L, name, sopt=subpix(), arrays=False, **big)[1] == name + ": too many corners"

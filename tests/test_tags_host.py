"""K27 (csrc/clc_tags.hpp: tag-grid corners from K25's candidates) on the host: the kernel header compiled with g++
(tests/shim/tags_shim.cpp, the threads as loops) against the numpy restatement tests/tags_ref.py, bit for bit on every output — every value
is an integer, or a NaN — on the scenes of tests/tags_cases.py; what the scenes are required to show, on the restatement alone; the
symbols, the structs, the argument checks of the product library without a device; TagFamily.generate; and the header under
AddressSanitizer and UBSan in two stand-alone programs."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import chess_ref  # noqa: E402
import subpix_cases as sp  # noqa: E402
import tags_cases as cases  # noqa: E402
import tags_ref as ref  # noqa: E402
from camlasercalibratool_amd import _capi, TagFamily, chessboard_order  # noqa: E402


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    return cases.build_shims(str(tmp_path_factory.mktemp("tags")))


def test_structs_defaults_symbols(shims):
    assert shims[1].shim_tag_options_size() == C.sizeof(_capi.TagOptions) == 24
    assert shims[1].shim_tag_family_size() == C.sizeof(_capi.TagFamilyC) == 24
    d = _capi.default_tag_options()  # the library's own, no device needed
    assert (d.min_side_px, d.max_side_px, d.contrast, d.max_border_errors, d.max_quads, d.reserved) == (16, 0, 40, 0, 256, 0)
    assert ref.Options() == ref.Options(16, 0, 40, 0, 256)
    names = ["clc_tag_options_default", "clc_tag_grid", "clc_tag_grid_device", "clc_tag_grid_points_device"]
    header = open(os.path.join(ROOT, "include", "clc.h")).read()
    L = _capi.lib()
    for n in names:
        assert re.search(r"\b%s\(" % n, header) and n in _capi.EXPORTED and hasattr(L, n), n
    for n, v in (("CLC_TAG_MAX_QUADS", 1024), ("CLC_TAG_MAX_OUT", 4), ("CLC_TAG_MAX_TAGS", 1024), ("CLC_TAG_MAX_CODES", 4096), ("CLC_TAG_OK", 1),
                 ("CLC_TAG_OVERFLOW", -2)):
        assert re.search(r"#define %s +%d\b" % (n, v), header), n
    assert (_capi.TAG_MAX_QUADS, _capi.TAG_MAX_OUT, _capi.TAG_OK, _capi.TAG_OVERFLOW) == (1024, ref.MAX_OUT, ref.OK, ref.OVERFLOW)
    assert L.clc_version() == 210
    import camlasercalibratool_amd as pkg
    assert pkg.FindTagGridCorners and pkg.TagFamily and pkg.TagOptions is _capi.TagOptions
    assert all(hasattr(pkg.Solver, m) for m in ("tag_grid", "tag_grid_device", "tag_grid_points_device"))


def test_family_generate_is_repeatable_and_keeps_its_distance():
    for side, n, dist in ((4, 8, 5), (6, 64, 10), (3, 4, 3)):
        f = TagFamily.generate(side, n, dist, seed=27)
        g = TagFamily.generate(side, n, dist, seed=27)
        assert np.array_equal(f.codes, g.codes) and len(f.codes) == n and f.codes.dtype == np.uint64
        assert not np.array_equal(f.codes, TagFamily.generate(side, n, dist, seed=28).codes)
        assert all(int(c) >> (side * side) == 0 for c in f.codes)
        # brute force, with rotations written out cell by cell: the word read from the next corner has cell (r, c) = old cell (c, d - 1 - r)
        def turn(w):
            m = [[(w >> (side * side - 1 - (r * side + c))) & 1 for c in range(side)] for r in range(side)]
            out = 0
            for r in range(side):
                for c in range(side):
                    out = (out << 1) | m[c][side - 1 - r]
            return out
        ham = lambda a, b: bin(a ^ b).count("1")
        smallest = 99
        for i, a in enumerate(int(c) for c in f.codes):
            rots = [a, turn(a), turn(turn(a)), turn(turn(turn(a)))]
            assert turn(rots[3]) == a and rots == TagFamily.rotations(a, side)
            smallest = min([smallest] + [ham(a, r) for r in rots[1:]])
            for b in (int(c) for c in f.codes[i + 1:]):
                smallest = min([smallest] + [ham(b, r) for r in rots])
        assert smallest >= dist, (side, smallest)
    with pytest.raises(ValueError):
        TagFamily.generate(3, 64, 5, seed=1)


@pytest.mark.parametrize("name", cases.NAMES)
def test_what_the_scenes_are_required_to_show(name):
    """On the restatement alone: every tag fully in view (its corners >= 6 px inside the image) is decoded with its own id, each of its
    integer corners within 1.5 px of the truth, in the tag's own corner order; no tag is reported that is not there; no decode sample
    coordinate within 1e-9 of a half-integer."""
    s = cases.scene(name)
    ref.HALF.clear()
    cases.reference.cache_clear()
    r = cases.reference(name)
    assert ref.HALF and min(ref.HALF) > 1e-9, min(ref.HALF)
    cols, rows = s["grid"]
    seen = r["hamming"][0] >= 0
    assert r["status"][0] == ref.OK and r["count"][0] == seen.sum() and r["n_edges_dropped"][0] == 0
    drawn = list(s["ids"])
    for i in range(cols * rows):
        places = [k for k, v in enumerate(drawn) if v == i and s["in_view"][k]]
        if not places:
            assert not seen[i], (name, i)  # no tag that is not there (or not fully in view)
            continue
        assert seen[i], (name, i)
        err = min(np.linalg.norm(r["corners"][0, i] - s["truth"][k], axis=1).max() for k in places)
        print(name, "id", i, "hamming", r["hamming"][0, i], "corner error", err)
        assert err <= 1.5, (name, i, err)
    assert np.isnan(r["corners"][0][~seen]).all() and (r["hamming"][0][~seen] == -1).all()
    tag_side = np.linalg.norm(s["truth"][:, 1] - s["truth"][:, 0], axis=1)
    assert tag_side.min() >= 26.0, tag_side.min()
    if name == "cut_off":
        # the chessboard route needs the whole board: on this image's candidates no grid of the tags' corners is found
        assert s["in_view"].sum() == 5 and seen.sum() == 5
        det = chess_ref.detect(s["image"][None], s["width"], ref.CHESS)
        for grid in ((2 * cols, 2 * rows), (2 * rows, 2 * cols)):
            cut = dict(xy=det["xy"][:, :1024], count=det["count"])
            o = chessboard_order(cut["xy"], cut["count"], grid[0], grid[1], status=det["status"])
            assert o["status"][0] != chess_ref.FOUND, o["status"]
    if name.startswith("turn_"):
        assert r["n_quads"][0] == 1 and seen.all()
    if name == "family_64":
        assert len(s["family"].codes) == 64 and r["n_foreign"][0] == 0 and seen.all()
    if name == "foreign_id":
        assert r["n_foreign"][0] == 1 and list(np.flatnonzero(~seen)) == [2]
    if name == "id_twice":
        assert r["n_quads"][0] == 6 and r["n_foreign"][0] == 0 and list(np.flatnonzero(~seen)) == [4]


@pytest.mark.parametrize("name", cases.NAMES)
def test_shim_is_the_restatement_bit_for_bit(shims, name):
    s = cases.scene(name)
    cols, rows = s["grid"]
    want = cases.reference(name)
    img = s["image"][None]
    cases.assert_same_bits(cases.shim_tag_grid(shims, img, s["width"], s["family"], cols, rows), want, name)
    # the padding bytes behind each row change nothing
    for pitch, fill in ((s["width"] + 3, 201), (s["width"] + 17, 0)):
        cases.assert_same_bits(cases.shim_tag_grid(shims, sp.padded(img, pitch, fill=fill), s["width"], s["family"], cols, rows), want,
                               "%s (pitch %d)" % (name, pitch))


def test_batched_is_image_by_image(shims):
    """The four 3 x 2 scenes of one family in one call and in another order: each image's rows are its own."""
    names = ["big_3x2_d6_b2", "cut_off", "foreign_id", "id_twice"]
    fam = cases.scene(names[0])["family"]
    for order in ([0, 1, 2, 3], [3, 1, 0, 2, 1]):
        imgs = np.stack([cases.scene(names[k])["image"] for k in order])
        got = cases.shim_tag_grid(shims, imgs, 320, fam, 3, 2)
        want = ref.tag_grid(imgs, 320, cases.ref_family(fam), 3, 2)
        cases.assert_same_bits(got, want, "batch %s" % order)
        for j, k in enumerate(order):
            for key in cases.KEYS:
                assert np.array_equal(got[key][j], cases.reference(names[k])[key][0], equal_nan=True), (order, j, key)
    # the batches of the GPU tests: 160 x 120, decoded with the 4 x 4 family
    fam4 = cases.scene("small_2x2_d4_b2")["family"]
    got = cases.shim_tag_grid(shims, cases.batch(3), 160, fam4, 2, 2)
    cases.assert_same_bits(got, ref.tag_grid(cases.batch(3), 160, cases.ref_family(fam4), 2, 2), "batch of 3")
    assert list(got["count"]) == [4, 0, 4]
    empty = cases.shim_tag_grid(shims, cases.batch(0), 160, fam4, 2, 2)
    assert empty["corners"].shape == (0, 4, 4, 2)


def test_options_at_their_ends(shims):
    s = cases.scene("big_3x2_d6_b2")
    img, fam, rf = s["image"][None], s["family"], cases.ref_family(s["family"])
    def both(o, chess=ref.CHESS, image=img, width=320):
        want = ref.tag_grid(image, width, rf, 3, 2, o, chess)
        cases.assert_same_bits(cases.shim_tag_grid(shims, image, width, fam, 3, 2, o, chess), want, str(o))
        return want
    one = both(ref.Options(max_quads=1))
    assert one["n_quads"][0] == 6 and one["count"][0] == 1
    assert both(ref.Options(max_border_errors=8))["count"][0] == 6 and both(ref.Options(max_border_errors=0))["count"][0] == 6
    none = both(ref.Options(contrast=255))  # above the image's range: no edge, no tag
    assert none["count"][0] == 0 and none["n_quads"][0] == 0 and none["status"][0] == ref.OK and np.isnan(none["corners"]).all()
    assert both(ref.Options(min_side_px=60))["count"][0] == 0 and both(ref.Options(max_side_px=20))["count"][0] == 0
    few = both(ref.Options(), chess_ref.Options(max_per_image=8))  # the eight strongest candidates alone
    assert few["count"][0] <= 2
    # a white border cell: a tag whose border ring is broken is refused at 0 errors and read at 8
    broken = img.copy()
    quad = s["truth"][0]
    cx, cy = (0.9 * quad[0] + 0.1 * quad[2])  # inside the border ring, near corner 0
    broken[0, int(cy) - 1:int(cy) + 2, int(cx) - 1:int(cx) + 2] = 220
    strict, loose = both(ref.Options(max_border_errors=0), image=broken), both(ref.Options(max_border_errors=8), image=broken)
    print("broken border: seen at 0 errors", strict["hamming"][0], "at 8", loose["hamming"][0])
    assert loose["count"][0] == 6 and strict["count"][0] == 5 and strict["hamming"][0, 0] == -1  # tag 0 alone is refused
    # images without a domain (smaller than 11 x 11) and a single pixel
    for w, h in ((10, 10), (1, 1), (11, 9)):
        tiny = np.full((2, h, w), 99, np.uint8)
        r = both(ref.Options(), image=tiny, width=w)
        assert (r["count"] == 0).all() and (r["status"] == ref.OK).all()
    # a detection that overflowed: the status, and no tag
    noise = np.random.default_rng(2502).integers(0, 256, (1, 400, 640), dtype=np.uint8)
    over = both(ref.Options(), chess_ref.Options(threshold=1, nms_radius=1, max_per_image=1024), image=noise, width=640)
    assert over["status"][0] == ref.OVERFLOW and over["count"][0] == 0 and over["n_quads"][0] == 0


def test_edge_list_full(shims):
    """CLC_TAG_MAX_OUT reached on the crafted image: the first four passing edges of a candidate in increasing slot are kept, the others
    counted."""
    img, fam, o = cases.fence()
    want = ref.tag_grid(img, 300, cases.ref_family(fam), 1, 1, o)
    assert want["n_edges_dropped"][0] > 0 and want["count"][0] == 0
    cases.assert_same_bits(cases.shim_tag_grid(shims, img, 300, fam, 1, 1, o), want, "fence")


def test_compaction(shims):
    names = ["big_3x2_d6_b2", "cut_off", "foreign_id", "id_twice"]
    r = {k: np.concatenate([cases.reference(n)[k] for n in names] + [cases.reference(names[0])[k] * 0 - 1 if k == "hamming" else
                                                                  cases.reference(names[0])[k]]) for k in ("corners", "hamming")}
    px, bd, off = cases.shim_points(shims, r["corners"], r["hamming"], 3, 2, 0.055, 0.3)
    wpx, wbd, woff = ref.points(r["corners"], r["hamming"], 3, 2, 0.055, 0.3)
    assert list(off) == list(woff) == [0, 24, 44, 64, 84, 84]
    assert np.array_equal(px[:84].view(np.uint8), wpx.view(np.uint8)) and np.array_equal(bd[:84].view(np.uint8), wbd.view(np.uint8))
    assert (px[84:] == -7).all() and (bd[84:] == -7).all()
    assert np.allclose(wbd[4:8], np.array([[1, 0], [1, 0], [1, 0], [1, 0]]) * 0.0715 + np.array([[0, 0], [0.055, 0], [0.055, 0.055], [0, 0.055]]))


def tag_call(L, name, fam=None, topt=None, copt=None, sopt=None, images=True, width=16, height=16, pitch=16, n=1, cols=2, rows=2, arrays=True,
             handle=None):
    V = lambda a: a.ctypes.data_as(C.c_void_p)
    img = np.zeros((1, 16, 16), np.uint8)
    out = cases.empty_result(1, 1024)
    ref_ = lambda o: C.byref(o) if o is not None else None
    a = [V(out[k]) if arrays else None for k in ("corners", "hamming", "count", "status")]
    code = getattr(L, name)(handle, ref_(fam), ref_(topt), ref_(copt), ref_(sopt), V(img) if images else None, width, height, pitch, n, cols, rows,
                            a[0], a[1], a[2], a[3], None, None, None, None)
    return code, L.clc_last_error().decode()


@pytest.mark.parametrize("name", ["clc_tag_grid", "clc_tag_grid_device"])
def test_refusals_of_arguments(name):
    """Every CLC_ERR_INVALID_ARG through the product library, before any device work (there is no device here, and no handle)."""
    from camlasercalibratool_amd import _build
    L = _capi.load(_build.PRODUCT_LIB_PATH)
    f = cases.family(4)
    def fam(**kw):
        c = f.c_struct()
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    def topt(**kw):
        o = _capi.default_tag_options()
        for k, v in kw.items():
            setattr(o, k, v)
        return o
    high = np.array([1 << 16], np.uint64)
    bad_chess = _capi.ChessOptions(500, 9, 250, 256, 0)
    bad_subpix = _capi.SubpixOptions(0, 3, -1, -1, 30, 0, 0.1)
    cases_ = [(dict(fam=None), "family"), (dict(fam=fam(side=2)), "side"), (dict(fam=fam(side=8)), "side"), (dict(fam=fam(border=0)), "border"),
              (dict(fam=fam(border=3)), "border"), (dict(fam=fam(n_codes=0)), "n_codes"), (dict(fam=fam(n_codes=4097)), "n_codes"),
              (dict(fam=fam(max_hamming=-1)), "max_hamming"), (dict(fam=fam(max_hamming=9)), "max_hamming"), (dict(fam=fam(codes=None)), "codes"),
              (dict(fam=fam(codes=high.ctypes.data, n_codes=1)), "bits above"),
              (dict(topt=topt(min_side_px=7)), "min_side_px"), (dict(topt=topt(max_side_px=15)), "max_side_px"), (dict(topt=topt(max_side_px=-1)), "max_side_px"),
              (dict(topt=topt(contrast=0)), "contrast"), (dict(topt=topt(contrast=256)), "contrast"), (dict(topt=topt(max_border_errors=-1)), "max_border_errors"),
              (dict(topt=topt(max_border_errors=9)), "max_border_errors"), (dict(topt=topt(max_quads=0)), "max_quads"), (dict(topt=topt(max_quads=1025)), "max_quads"),
              (dict(topt=topt(reserved=1)), "reserved"), (dict(cols=0), "cols and rows"), (dict(rows=0), "cols and rows"), (dict(cols=33, rows=32), "cols and rows"),
              (dict(copt=bad_chess), "nms_radius"), (dict(width=0), "width and height"), (dict(pitch=15), "pitch"), (dict(sopt=bad_subpix), "refinement"),
              (dict(images=False), "bad argument"), (dict(arrays=False), "bad argument"), (dict(), "bad argument")]  # (the last: no handle)
    for kw, text in cases_:
        kw.setdefault("fam", fam())
        code, msg = tag_call(L, name, **kw)
        assert code == -1 and msg.startswith(name + ":") and text in msg, (kw, code, msg, text)
    assert tag_call(L, name, fam=fam(), n=0, images=False, arrays=False)[0] == -1  # no image, but no handle either
    # every field of the refinement options, the order of two refusals, the corner count: the rows all composite forms share
    import imagecall_refusals
    imagecall_refusals.check_composite_refusals(L, name)
    V = C.c_void_p
    for args, text in [((None, None, 1, 0, 2, 0.05, 0.3, None, None, V(8)), "cols and rows"), ((None, None, 1, 2, 2, 0.0, 0.3, None, None, V(8)), "tag_size"),
                       ((None, None, 1, 2, 2, 0.05, -0.1, None, None, V(8)), "tag_spacing"), ((None, None, 1, 2, 2, float("nan"), 0.3, None, None, V(8)), "tag_size"),
                       ((None, None, 1, 2, 2, 0.05, 0.3, None, None, None), "bad argument"), ((V(8), V(8), 1, 2, 2, 0.05, 0.3, V(8), V(8), V(8)), "bad argument")]:
        code = L.clc_tag_grid_points_device(None, *args)
        msg = L.clc_last_error().decode()
        assert code == -1 and msg.startswith("clc_tag_grid_points_device:") and text in msg, (args, code, msg)


@pytest.mark.parametrize("program,needle", [("tags_sanitize_main.cpp", "images "), ("tags_quads_main.cpp", "quads ")])
def test_header_under_the_sanitizers(tmp_path, program, needle):
    """tests/shim/tags_sanitize_main.cpp (the edge and decode stages on images from 1 x 1 to 130 x 35 in exact allocations at every offset
    from a word boundary) and tests/shim/tags_quads_main.cpp (quads whose samples leave the image, edge lists and candidate lists at their
    ends), built with -fsanitize=address,undefined and run as ordinary processes."""
    exe = str(tmp_path / "prog")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "shim", program), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    assert needle in p.stdout, p.stdout[-2000:]

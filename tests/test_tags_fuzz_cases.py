"""The K27 fuzz cases (tests/tags_fuzz_cases.py) without a GPU: what every scene is required to show, on the restatement
(tests/tags_ref.py) alone — a scene that does not show its property fails here, and tests/test_gpu_tags_fuzz.py runs the same scenes on
the device against the host build — and the host build (tests/shim/tags_shim.cpp behind tests/shim/chess_shim.cpp) against the
restatement, bit for bit on every output.

Near-ties.  Candidates are integer pixels, so the cell centres of a small quad often fall on exact half-pixels, where the rounding of the
homography's elimination decides which pixel rint picks and the restatement's LAPACK solve may round the other way.  Every scene
here has no decoded quad with an undecidable sample (ref.AMBIGUOUS: within 1e-9 of a half-integer, and the pixels it may round to
not all inside the image and on one side of the threshold): where the coordinate is a tie, either pixel gives the same cell.

MEASURED holds what the restatement gave when the cases were made (candidates, quads, tags seen, highest accepted rank, edges dropped,
quads with a near-tie sample); the table of DESIGN.md K27 is a copy of it."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import tags_cases as cases  # noqa: E402
import tags_fuzz_cases as F  # noqa: E402
import tags_ref as ref  # noqa: E402

MEASURED = {
    "wide_9x8_d4_b1": (502, 71, 70, 70, 8, 16),
    "wide_9x7_d6_b2": (349, 58, 57, 56, 2, 9),
    "side_3_b1": (26, 6, 6, 5, 0, 0),
    "side_5_b2": (40, 6, 6, 5, 0, 0),
    "side_7_b2": (45, 7, 4, 6, 0, 1),
    "side_7_b1": (81, 6, 6, 5, 0, 0),
    "t4096_g65": (27, 6, 3, 3, 0, 1),
    "t4096_g128": (27, 6, 3, 3, 0, 1),
    "t4096_g1024": (27, 6, 4, 3, 0, 1),
    "t1000_g1024": (27, 6, 6, 5, 0, 1),
    "t17_g65": (27, 6, 6, 5, 0, 1),
    "t1_g65": (27, 6, 1, 4, 0, 1),
    "ties_g1024": (27, 6, 5, 4, 0, 1),
    "crowd_10": (524, 1298, 4, 3, 281, 101),
    "crowd_9_dim": (690, 599, 4, 598, 0, 1),
    "crowd_9_wide": (1024, 921, 4, 3, 0, 0),
    "crowd_9_cut": (316, 257, 4, 256, 0, 0),
}


@pytest.fixture(scope="module")
def shims(tmp_path_factory):
    return cases.build_shims(str(tmp_path_factory.mktemp("tagsfuzz")))


def measured(name, r):
    """The scene's record; no decoded quad is ambiguous."""
    got = (r["candidates"], r["n_quads"], r["count"], int(r["rank"].max()), r["n_edges_dropped"], r["near_ties"])
    print(name, "candidates %d, quads %d, tags seen %d, highest accepted rank %d, edges dropped %d, near-tie quads %d" % got, "of", r["decoded"],
          "decoded; ambiguous", r["ambiguous"])
    assert r["ambiguous"] == 0, (name, r["ambiguous"])
    assert r["status"] == ref.OK
    assert MEASURED[name] == got, (name, got)


def one(c, r):
    """The restatement's dict of one image as the arrays of Solver.tag_grid."""
    T = c["grid"][0] * c["grid"][1]
    out = dict(corners=r["corners"][None], hamming=r["hamming"][None], strength=np.full((1, T, 4), np.nan))
    for key in ("count", "status", "n_quads", "n_foreign", "n_edges_dropped"):
        out[key] = np.array([r[key]], np.int32)
    return out


def host_is_restatement(shims, c, r, what):
    cases.assert_same_bits(F.host(shims, c), one(c, r), what)


# ---------------------------------------------------------------------------------------------------------------------------------
# 1, 2
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.BOARDS)
def test_boards(shims, name):
    """The boards of more than 64 tags: more than 256 candidates (a second trip of the edge kernel's threads and of the candidates' load),
    and on the 9 x 8 one at least 65 tags seen with every id from 64 that is in view.  The payload sides 3, 5 and 7: every tag in view
    at Hamming 0.  On all of them: every tag seen has its own id's corners within 1.5 px of the truth, and no tag out of view is seen."""
    c = F.board(name)
    r = F.restated(c)
    measured(name, r)
    seen = r["hamming"] >= 0
    assert not (seen & ~c["in_view"]).any() and r["n_foreign"] == 0
    for i in np.flatnonzero(seen):
        err = np.linalg.norm(r["corners"][i] - c["truth"][i], axis=1).max()
        assert err <= 1.5 and r["hamming"][i] == 0, (name, i, err, r["hamming"][i])
    if name in F.WIDE_BOARDS:
        assert r["candidates"] >= 257 and r["n_edges_dropped"] > 0
        assert seen.sum() >= (65 if name == "wide_9x8_d4_b1" else 57)
        assert seen[64:][c["in_view"][64:]].all()
    else:
        assert c["in_view"].all() and seen.all()
    if name == "wide_9x8_d4_b1":
        assert c["in_view"][64:].sum() >= 8 and r["rank"].max() >= 64
    host_is_restatement(shims, c, r, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# 3
# ---------------------------------------------------------------------------------------------------------------------------------
def test_sparse_tables_hold_no_accident():
    """No random word of a table is within max_hamming of a drawn code under any rotation, and the drawn codes are that far from one
    another: what the image decodes to is what was planted."""
    drawn = [int(w) for w in F.sparse_scene()["drawn"].codes]
    turns = np.array([F.turned(w, k) for w in drawn for k in range(4)], dtype=np.uint64)
    for a in range(6):
        for b in range(a + 1, 6):
            assert min(bin(drawn[a] ^ F.turned(drawn[b], k)).count("1") for k in range(4)) > 2, (a, b)
    for name, (n, _, placed) in F.SPARSE.items():
        codes = F.sparse_table(name).codes
        assert len(codes) == n and F.sparse_table(name).max_hamming == 1
        free = np.array([i for i in range(n) if i not in placed], dtype=np.int64)
        x = codes[free][:, None] ^ turns[None, :]
        pop = np.zeros(x.shape, np.int64)
        for k in range(36):
            pop += ((x >> np.uint64(k)) & np.uint64(1)).astype(np.int64)
        assert pop.size == 0 or pop.min() > 1, (name, pop.min())


# name -> ({id seen: drawn code}, n_foreign)
SPARSE_WANT = {
    "t4096_g65": ({0: 0, 63: 1, 64: 2}, 3),
    "t4096_g128": ({15: 0, 16: 1, 127: 2}, 3),
    "t4096_g1024": ({511: 0, 512: 1, 1023: 2, 17: 4}, 2),
    "t1000_g1024": ({0: 0, 63: 1, 64: 2, 999: 3, 496: 4, 497: 5}, 0),
    "t17_g65": ({0: 5, 15: 4, 16: 3, 1: 2, 2: 1, 3: 0}, 0),
    "t1_g65": ({0: 3}, 0),
    "ties_g1024": ({70: 3, 300: 0, 600: 1, 900: 2, 1000: 4}, 1),
}


@pytest.mark.parametrize("name", F.SPARSE)
def test_sparse_ids(shims, name):
    """Exactly the planted outcome: the drawn codes come back at the ids the table holds them at, with the drawn tag's corners; an id
    from cols x rows on is counted as foreign; of a code at two ids the smaller id is seen, whatever rotation it holds the code in; a
    code equal to its own half turn is read at the smaller of its two rotations."""
    c, s = F.sparse_case(name), F.sparse_scene()
    assert s["in_view"].all()
    r = F.restated(c)
    measured(name, r)
    want, foreign = SPARSE_WANT[name]
    seen = np.flatnonzero(r["hamming"] >= 0)
    assert sorted(seen) == sorted(want) and r["n_foreign"] == foreign and r["n_quads"] == 6 and r["count"] == len(want)
    assert len(c["family"].codes) == F.SPARSE[name][0] and c["grid"][0] * c["grid"][1] in (65, 128, 1024)
    for i, k in want.items():
        assert r["hamming"][i] == 0
        turns = F.SPARSE[name][2][i][1]
        # the table holds the drawn code turned: the corners come back turned by as much
        err = min(np.linalg.norm(r["corners"][i] - np.roll(s["truth"][k], j, axis=0), axis=1).max() for j in ((-turns) % 4, turns % 4))
        assert err <= 1.5, (name, i, err)
    if name == "ties_g1024":
        # X (300 .. 303) and Y (600 .. 603) are accepted at a rotation other than 0, so an order (Hamming, rotation, id) would pick
        # another id; S reads the same at its rotation and two on
        assert r["rotation"][300] != 0 and r["rotation"][600] != 0 and r["rotation"][900] in (0, 1)
    host_is_restatement(shims, c, r, name)


# ---------------------------------------------------------------------------------------------------------------------------------
# 4
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", F.CROWDS)
def test_crowds(shims, name):
    """The 2 x 2 board inside a chequer: all four tags at Hamming 0 among more than 256 candidates, and no square of the texture decodes
    (its payload reads all dark or all light, more than max_hamming from every code).  crowd_10: more than 512 candidates, more than
    1024 quads with the cap inside one p0's paths, a p0 of three or more paths, dropped edges.  crowd_9_dim: the tags behind more than
    512 quads of the texture.  crowd_9_wide: every candidate slot taken.  crowd_9_cut: the tags at the ranks 253 .. 256."""
    c = F.crowd(name)
    r = F.restated(c)
    measured(name, r)
    fam = cases.ref_family(c["family"])
    assert all(bin(int(w)).count("1") > fam.max_hamming and bin(int(w) ^ 0xFFFF).count("1") > fam.max_hamming for w in fam.codes)  # no square decodes
    assert r["count"] == 4 and (r["hamming"] == 0).all() and r["n_foreign"] == 0 and r["candidates"] > 256
    paths = F.paths_per_p0(r["quads"])
    Q = r["quads"]
    if name == "crowd_10":
        assert r["candidates"] > 512 and r["n_quads"] > 1024 and r["n_edges_dropped"] > 0
        assert Q[1023][0] == Q[1024][0]      # the cap falls inside the paths of one p0
        assert max(paths.values()) >= 3
    if name == "crowd_9_dim":
        assert r["candidates"] > 512 and r["rank"].min() >= 512
    if name == "crowd_9_wide":
        # every slot taken (the detection found more, and hands on the strongest CLC_CHESS_MAX_CANDIDATES): the last trip of every
        # thread of the edge kernel and of every lane of the candidates' load
        assert r["raw"] > 1024 and r["candidates"] == F.MAX_CAND == 1024 and r["n_quads"] > 512
    if name == "crowd_9_cut":
        assert sorted(r["rank"]) == [253, 254, 255, 256] and 256 <= r["rank"].max() < 512
    host_is_restatement(shims, c, r, name)


@pytest.mark.parametrize("max_quads", F.MAX_QUADS)
def test_crowd_cut_anywhere(shims, max_quads):
    """crowd_9_cut, whose four tags have the ranks 253 .. 256: max_quads 255, 256, 257 and the default see two, three, four and three
    of them; and the list cut one short of each tag's quad and at it."""
    c = F.crowd("crowd_9_cut", max_quads if max_quads else ref.Options().max_quads)
    assert c["options"].max_quads == (max_quads or 256)
    r = F.restated(c)
    assert r["ambiguous"] == 0 and r["n_quads"] == 257
    seen = r["hamming"] >= 0
    assert list(seen) == list(F.restated(F.crowd("crowd_9_cut"))["rank"] < c["options"].max_quads)
    assert r["count"] == {253: 0, 254: 1, 255: 2, 256: 3, 257: 4, 0: 3}[max_quads]
    # the host build keeps its quad list from call to call, as a workgroup finds LDS as another left it: the call before leaves another
    # image's quads in it, so that a quad decoded without having been stored is not this image's
    other = F.crowd("crowd_9_dim")
    assert F.host(shims, other)["n_quads"][0] == MEASURED["crowd_9_dim"][1] > 257
    host_is_restatement(shims, c, r, "crowd_9_cut at max_quads %d" % max_quads)


def test_crowd_cap_inside_a_p0(shims):
    """crowd_10 cut where one p0 has several paths, in the middle of them: the quads before the cut are decoded, those behind it are
    counted alone."""
    full = F.restated(F.crowd("crowd_10"))
    Q = full["quads"]
    at = next(k for k in range(2, len(Q)) if Q[k - 2][0] == Q[k - 1][0] == Q[k][0])
    assert F.CAP_INSIDE == (at - 1, at, at + 1, 1023) and len({q[0] for q in Q[at - 2:at + 2]}) == 1 and len({q[0] for q in Q[1022:1026]}) == 1
    for max_quads in F.CAP_INSIDE:
        c = F.crowd("crowd_10", max_quads)
        r = F.restated(c)
        assert r["n_quads"] == full["n_quads"] and r["ambiguous"] == 0
        assert list(r["hamming"] >= 0) == list(full["rank"] < max_quads)
        host_is_restatement(shims, c, r, "crowd_10 at max_quads %d" % max_quads)
    # the list full to its last slot with more quads behind it, and the ids 0 .. 3 of the grid not in the image (the per-id keys
    # stand behind the quad list in the kernel's LDS): they stay not seen
    c = F.crowd("crowd_10", 1024, shifted=True)
    r = F.restated(c)
    assert r["n_quads"] > 1024 and r["ambiguous"] == 0 and list(np.flatnonzero(r["hamming"] >= 0)) == [4, 5, 6, 7] and r["n_foreign"] == 0
    host_is_restatement(shims, c, r, "crowd_10, the ids 4 .. 7")


# ---------------------------------------------------------------------------------------------------------------------------------
# 5
# ---------------------------------------------------------------------------------------------------------------------------------
def test_batch_of_unlike_images(shims):
    """The nine distinct images on the restatement and the host build; then the 172 in one call on the host build: every image's rows
    are those of its kind alone, whatever stands beside it; once more under a pitch of width + 3."""
    c = F.batch_case()
    want = F.restated_result(c)
    kinds = {k: i for i, k in enumerate(F.KINDS)}
    for k, i in kinds.items():
        r = F.restated(c, i)
        assert r["ambiguous"] == 0, k
        print(k, "candidates", r["candidates"], "quads", r["n_quads"], "seen", r["count"])
    cand = {k: F.restated(c, i)["candidates"] for k, i in kinds.items()}
    assert cand["blank"] == 0 and cand["one"] == 1 and cand["three"] == 3 and min(cand["crowd_10"], cand["crowd_9_dim"]) > 512
    o = kinds["overflow"]
    assert want["status"][o] == ref.OVERFLOW and want["count"][o] == 0 and want["n_quads"][o] == 0 and np.isnan(want["corners"][o]).all()
    assert (np.delete(want["status"], o) == ref.OK).all()
    assert [want["count"][kinds[k]] for k in ("crowd_10", "crowd_9_dim", "crowd_9_cut", "board", "small")] == [4, 4, 4, 4, 4]
    single = F.host(shims, c)
    cases.assert_same_bits(single, want, "the distinct images")
    for i in range(len(F.KINDS)):  # each alone
        cases.assert_same_bits(F.host(shims, c, c["images"][i:i + 1]), {k: v[i:i + 1] for k, v in want.items()}, F.KINDS[i])
    order = F.batch_order()
    assert len(order) == F.BATCH_N == F.BATCH_CHUNK + 2 and list(order).count(o) == 1 and order[F.OVERFLOW_AT] == o
    assert order[0] == kinds["crowd_9_dim"] and order[F.BATCH_CHUNK] == kinds["blank"] and order[1] == kinds["three"]
    assert order[F.BATCH_CHUNK + 1] == kinds["crowd_10"]
    images = c["images"][order]
    expect = {k: v[order] for k, v in want.items()}
    cases.assert_same_bits(F.host(shims, c, images), expect, "172 images")
    import subpix_cases as sp
    cases.assert_same_bits(F.host(shims, c, sp.padded(images, F.BIG[0] + 3, fill=201)), expect, "172 images, pitch 323")


# ---------------------------------------------------------------------------------------------------------------------------------
# 6
# ---------------------------------------------------------------------------------------------------------------------------------
def test_compaction_cases_cover_what_they_should():
    assert {c[0] for c in F.COMPACTIONS} == {1, 63, 64, 65, 128, 1000, 1024}
    assert {c[2] for c in F.COMPACTIONS} >= {0, 1, 255, 256, 257, 513}
    assert {c[3] for c in F.COMPACTIONS} == set(F.PATTERNS)
    assert all(t % cols == 0 for t, cols, _, _ in F.COMPACTIONS) and any(64 % cols for _, cols, _, _ in F.COMPACTIONS)


@pytest.mark.parametrize("n_tags,cols,n_images,pattern", F.COMPACTIONS)
def test_compaction(shims, n_tags, cols, n_images, pattern):
    """shim_tag_points against ref.points: the same bytes in all three outputs, nothing written behind the last point."""
    corners, hamming = F.compaction(n_tags, cols, n_images, pattern)
    seen = hamming >= 0
    if pattern == "one_per_block":
        assert (seen.sum(axis=1) == -(-n_tags // 64)).all()
    if pattern == "half" and seen.size >= 64:
        assert 0.3 < seen.mean() < 0.7
    px, bd, off = cases.shim_points(shims, corners, hamming, cols, n_tags // cols, F.TAG_SIZE, F.TAG_SPACING)
    wpx, wbd, woff = ref.points(corners, hamming, cols, n_tags // cols, F.TAG_SIZE, F.TAG_SPACING)
    m = 4 * int(seen.sum())
    assert off.dtype == woff.dtype and np.array_equal(off, woff) and off[-1] == m
    assert np.array_equal(px[:m].view(np.uint8), wpx.view(np.uint8)) and np.array_equal(bd[:m].view(np.uint8), wbd.view(np.uint8))
    assert (px[m:] == -7).all() and (bd[m:] == -7).all()

"""Timing of clc_tag_grid_device (K27: tag-grid corners from images) whole — detection, edges, quads and decode, refinement at
half-window 3 — and without the refinement, beside clc_chess_corners_device (K25's detection, its first stage) and
clc_corner_subpix_device at half-window 3 on the corners it finds, on the same images in the same run: 10^4 images of 752 x 480
resident on the device showing a 6 x 6 grid of tags (144 corners; four rendered views in turn, a generated 6 x 6 family of 36 codes,
border 2), default options; warm medians.  Prints one JSON line; `python scripts/tag_grid.py [reps] [--images N] [--profile]`
(--profile: three whole calls and nothing else, for a run under `rocprofv3 --kernel-trace --stats`, which gives each kernel's own
time; profiles/tag_grid.md)."""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import camlasercalibratool_amd as clc  # noqa: E402
from camlasercalibratool_amd import _capi  # noqa: E402
import campose_ref  # noqa: E402
import tags_cases  # noqa: E402

WIDTH, HEIGHT, GRID, PROJ = 752, 480, (6, 6), (600.0, 600.0, 375.5, 239.5)
TAG_SIZE, TAG_PX = 0.055, 46.0
VIEWS = ((0.05, 0.1, -0.1), (-0.3, -0.15, 0.1), (3.0, 0.1, 0.2), (1.5, 0.0, 0.0))  # spin, tilt about x, tilt about y


def family():
    return clc.TagFamily.generate(6, 36, 10, seed=2736)


def scenes():
    fam = family()
    out = []
    for k, (spin, tx, ty) in enumerate(VIEWS):
        rng = np.random.default_rng(2740 + k)
        R = campose_ref.rotvec_to_R(np.array([0.0, 0.0, spin])) @ campose_ref.rotvec_to_R(np.array([tx, ty, 0.0])) @ tags_cases.FRONT
        period = TAG_SIZE * (1.0 + tags_cases.SPACING)
        centre = np.array([(5 * period + TAG_SIZE) / 2, (5 * period + TAG_SIZE) / 2, 0.0])
        z = TAG_SIZE * PROJ[0] / TAG_PX
        out.append(tags_cases.render_taggrid(WIDTH, HEIGHT, PROJ, GRID, TAG_SIZE, fam, tuple(range(36)), R, np.array([0.0, 0.0, z]) - R @ centre, rng))
    return out


def _ms(f):
    t0 = time.perf_counter()
    f()
    return (time.perf_counter() - t0) * 1e3


def main():
    import torch
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    reps = int(args[0]) if args else 7
    profile = "--profile" in sys.argv
    n = int(sys.argv[sys.argv.index("--images") + 1]) if "--images" in sys.argv else 10000
    sc, fam = scenes(), family()
    cols, rows = GRID
    T = cols * rows
    dev = torch.device("cuda:0")
    base = torch.from_numpy(np.stack([s["image"] for s in sc])).to(dev)
    images = base.repeat((n + len(sc) - 1) // len(sc), 1, 1)[:n].contiguous()
    co = _capi.default_chess_options()
    co.max_per_image = 1024  # what clc_tag_grid_device runs the detection with
    d_xy = torch.empty((n, 1024, 2), dtype=torch.float32, device=dev)
    d_cc = torch.empty(n, dtype=torch.int32, device=dev); d_cs = torch.empty_like(d_cc)
    d_corners = torch.empty((n, T, 4, 2), dtype=torch.float32, device=dev); d_ham = torch.empty((n, T), dtype=torch.int32, device=dev)
    d_count = torch.empty_like(d_cc); d_status = torch.empty_like(d_cc); d_quads = torch.empty_like(d_cc); d_foreign = torch.empty_like(d_cc)
    d_dropped = torch.empty_like(d_cc)
    d_lam = torch.empty((n, T, 4), dtype=torch.float64, device=dev)
    d_refined = torch.empty_like(d_corners)
    d_off = (torch.arange(n + 1, dtype=torch.int64, device=dev) * 4 * T).contiguous()
    torch.cuda.synchronize()
    out = {"what": "clc_tag_grid_device (whole, and without refinement), clc_chess_corners_device, clc_corner_subpix_device (half-window 3); warm median ms",
           "images": n, "image": [WIDTH, HEIGHT], "grid": list(GRID), "reps": reps}
    so = _capi.default_subpix_options(3)
    with clc.Solver(0) as sv:
        def whole(sopt=so):
            sv.tag_grid_device(images.data_ptr(), WIDTH, HEIGHT, WIDTH, n, fam, cols, rows, d_corners.data_ptr(), d_ham.data_ptr(), d_count.data_ptr(),
                               d_status.data_ptr(), d_quads.data_ptr(), d_foreign.data_ptr(), d_dropped.data_ptr(), d_lam.data_ptr(), None, None, sopt)

        def detect():
            sv.chess_corners_device(images.data_ptr(), WIDTH, HEIGHT, WIDTH, n, d_xy.data_ptr(), d_cc.data_ptr(), d_cs.data_ptr(), 0, 0, co)

        def refine():
            sv.corner_subpix_device(images.data_ptr(), WIDTH, HEIGHT, WIDTH, n, d_corners.data_ptr(), d_off.data_ptr(), d_refined.data_ptr(), 0, 0,
                                    d_lam.data_ptr(), so)

        whole()  # warm
        if profile:
            for _ in range(3):
                whole()
            print(json.dumps({"profile": True, "images": n}))
            return
        tw = [_ms(whole) for _ in range(reps)]
        whole(None)
        tp = [_ms(lambda: whole(None)) for _ in range(reps)]  # leaves the integer corners in d_corners: the refinement's starts below
        detect()
        td = [_ms(detect) for _ in range(reps)]
        refine()
        tr = [_ms(refine) for _ in range(reps)]
        count, quads, cand = d_count.cpu().numpy(), d_quads.cpu().numpy(), d_cc.cpu().numpy()
        med = statistics.median
        out.update({
            "tag_grid_ms": round(med(tw), 3), "tag_grid_ms_min_max": [round(min(tw), 3), round(max(tw), 3)],
            "tag_grid_no_refinement_ms": round(med(tp), 3), "tag_grid_no_refinement_ms_min_max": [round(min(tp), 3), round(max(tp), 3)],
            "detect_ms": round(med(td), 3), "detect_ms_min_max": [round(min(td), 3), round(max(td), 3)],
            "subpix3_ms": round(med(tr), 3), "subpix3_ms_min_max": [round(min(tr), 3), round(max(tr), 3)],
            "edges_and_decode_ms_by_difference": round(med(tp) - med(td), 3),
            "tags_per_image_min_max": [int(count.min()), int(count.max())], "quads_per_image_min_max": [int(quads.min()), int(quads.max())],
            "candidates_per_image_min_max": [int(cand.min()), int(cand.max())], "edges_dropped": int(d_dropped.sum().item()),
            "foreign": int(d_foreign.sum().item()),
        })
    print(json.dumps(out))


if __name__ == "__main__":
    main()

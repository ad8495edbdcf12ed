"""Camera models and calibration-board geometry of the reference's camera side (CamPoseEst, src/calcCamPose.cpp).

Camera: the two camodocal models the reference's nodes select (PINHOLE, KANNALA_BRANDT), read from the reference's OpenCV-YAML
config files; ClcCamera: its C layout (include/clc.h clc_camera).  The board helpers restate the board-frame corner coordinates
(cv::Point3f, z = 0) of calcCamPose.cpp in its corner order."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

PINHOLE = 1          # CLC_CAMERA_PINHOLE
KANNALA_BRANDT = 2   # CLC_CAMERA_KANNALA_BRANDT


class ClcCamera(C.Structure):
    """clc_camera (include/clc.h), 72 bytes."""
    _fields_ = [("model", C.c_int32), ("reserved", C.c_int32), ("proj", C.c_double * 4), ("dist", C.c_double * 4)]


@dataclass(frozen=True)
class Camera:
    """model: PINHOLE (proj = fx fy cx cy, dist = k1 k2 p1 p2) or KANNALA_BRANDT (proj = mu mv u0 v0, dist = k2 k3 k4 k5)."""
    model: int
    proj: Tuple[float, float, float, float]
    dist: Tuple[float, float, float, float]
    width: int = 0
    height: int = 0

    @staticmethod
    def pinhole(fx, fy, cx, cy, k1=0.0, k2=0.0, p1=0.0, p2=0.0, width=0, height=0) -> "Camera":
        return Camera(PINHOLE, (float(fx), float(fy), float(cx), float(cy)), (float(k1), float(k2), float(p1), float(p2)), width, height)

    @staticmethod
    def kannala_brandt(mu, mv, u0, v0, k2=0.0, k3=0.0, k4=0.0, k5=0.0, width=0, height=0) -> "Camera":
        return Camera(KANNALA_BRANDT, (float(mu), float(mv), float(u0), float(v0)), (float(k2), float(k3), float(k4), float(k5)),
                      width, height)

    @staticmethod
    def from_yaml(path: str) -> "Camera":
        """The camera of one of the reference's config files (%YAML:1.0, model_type, projection_parameters /
        distortion_parameters blocks): `key: value` lines, the block members indented under their block."""
        top, blocks, block = {}, {}, None
        with open(path) as f:
            for raw in f:
                line = raw.split("#", 1)[0].rstrip()
                if not line.strip() or line.startswith("%") or line.strip() == "---":
                    continue
                indented = line[0] in " \t"
                key, sep, val = line.strip().partition(":")
                if not sep:
                    continue
                key, val = key.strip(), val.strip().strip('"').strip("'")
                if not indented:
                    block = None
                    if val == "":
                        block = key
                        blocks[block] = {}
                    else:
                        top[key] = val
                elif block is not None:
                    blocks[block][key] = val
        kv = {}
        for b in ("projection_parameters", "distortion_parameters"):
            kv.update({k: float(v) for k, v in blocks.get(b, {}).items()})
        model = top.get("model_type", "").upper()
        w, h = int(float(top.get("image_width", 0))), int(float(top.get("image_height", 0)))
        g = lambda k: kv.get(k, 0.0)
        if model == "PINHOLE":
            return Camera.pinhole(g("fx"), g("fy"), g("cx"), g("cy"), g("k1"), g("k2"), g("p1"), g("p2"), w, h)
        if model == "KANNALA_BRANDT":
            return Camera.kannala_brandt(g("mu"), g("mv"), g("u0"), g("v0"), g("k2"), g("k3"), g("k4"), g("k5"), w, h)
        raise ValueError(f"{path}: model_type {model!r} is not supported (PINHOLE, KANNALA_BRANDT)")

    def to_yaml(self, path: str, camera_name: str = "cam0") -> None:
        """Writes the camera in the reference's config format, the one from_yaml reads (%YAML:1.0, model_type, image size, the
        projection_parameters / distortion_parameters blocks; Kannala-Brandt keeps all eight under projection_parameters, as the
        reference's file does).  repr() of a float round-trips: from_yaml returns an equal Camera."""
        if self.model == PINHOLE:
            blocks = [("distortion_parameters", zip(("k1", "k2", "p1", "p2"), self.dist)),
                      ("projection_parameters", zip(("fx", "fy", "cx", "cy"), self.proj))]
            name = "PINHOLE"
        elif self.model == KANNALA_BRANDT:
            blocks = [("projection_parameters", zip(("mu", "mv", "u0", "v0", "k2", "k3", "k4", "k5"), tuple(self.proj) + tuple(self.dist)))]
            name = "KANNALA_BRANDT"
        else:
            raise ValueError(f"model {self.model!r} is not supported (PINHOLE, KANNALA_BRANDT)")
        lines = ["%YAML:1.0", "", "#camera calibration", f"model_type: {name}", f"camera_name: {camera_name}",
                 f"image_width: {int(self.width)}", f"image_height: {int(self.height)}"]
        for block, items in blocks:
            lines += ["", f"{block}:"] + [f"   {k}: {float(v)!r}" for k, v in items]
        with open(path, "w") as f:
            f.write("\n".join(lines) + "\n")

    def to_c(self) -> ClcCamera:
        c = ClcCamera()
        c.model = self.model
        c.reserved = 0
        for i in range(4):
            c.proj[i] = self.proj[i]
            c.dist[i] = self.dist[i]
        return c


def kalibr_board_points(ids: Sequence[int], rows: int, cols: int, tag_size: float, tag_spacing: float) -> np.ndarray:
    """The four corners of every detected Kalibr tag id, in detection order (calcCamPose.cpp:115-141): tag (row, col) =
    (id / cols, id % cols), tag_spacing_sz = tag_sz (1 + spacing), corners (0,0) (sz,0) (sz,sz) (0,sz) from the tag's origin.
    float32 [4 len(ids), 2] (cv::Point3f; z = 0)."""
    s = tag_size * (1.0 + tag_spacing)  # rows: the board's size; the ids alone place the tags
    out = []
    for i in ids:
        r, c = int(i) // cols, int(i) % cols
        x0, y0 = s * c, s * r
        out += [(x0, y0), (x0 + tag_size, y0), (x0 + tag_size, y0 + tag_size), (x0, y0 + tag_size)]
    return np.array(out, dtype=np.float32).reshape(-1, 2)


def apriltag_points(tag_size: float) -> np.ndarray:
    """The single AprilTag's four corners (calcCamPose.cpp:189-203), float32 [4, 2]."""
    s = tag_size
    return np.array([(0.0, 0.0), (s, 0.0), (s, s), (0.0, s)], dtype=np.float32)


def chessboard_points(rows: int, cols: int, square: float) -> np.ndarray:
    """The chessboard's inner corners, row-major (calcCamPose.cpp:28-35: (j square, i square)), float32 [rows cols, 2]."""
    return np.array([(j * square, i * square) for i in range(rows) for j in range(cols)], dtype=np.float32).reshape(-1, 2)

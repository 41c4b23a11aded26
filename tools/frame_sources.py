"""Frame sources shared by the command-line drivers (tools/style_transfer_amd.py, tools/smooth_parsing_map_amd.py).

The reference's readers are optional third-party packages that an MI355X serving image need not carry:
    *.mp4 / *.avi / *.jpg / *.png  -> cv2 (when importable), frames BGR as VideoCapture.read() delivers them
    *.npy                          -> (N,H,W,3) uint8 array (memory-mapped), channel order given by the caller
    a directory                    -> sorted *.npy frames (H,W,3) uint8
"""
from __future__ import annotations

import os

import numpy as np

VIDEO_EXT = (".mp4", ".avi", ".mov", ".mkv", ".webm")
IMAGE_EXT = (".jpg", ".jpeg", ".png", ".bmp")


class NpySource:
    """(N,H,W,3) uint8 .npy, memory-mapped; random access, so every rank reads only its shard."""
    kind = "npy"

    def __init__(self, path, bgr):
        self.a = np.load(path, mmap_mode="r")
        if self.a.ndim == 3:
            self.a = self.a[None]
        if self.a.ndim != 4 or self.a.shape[3] != 3 or self.a.dtype != np.uint8:
            raise ValueError(f"{path}: expected (N,H,W,3) uint8 frames")
        self.bgr, self.fps = bgr, 25.0

    def __len__(self):
        return self.a.shape[0]

    def frames(self, start, stop):
        for i in range(start, stop):
            yield np.ascontiguousarray(self.a[i])


class DirSource:
    kind = "dir"

    def __init__(self, path, bgr):
        self.files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".npy"))
        if not self.files:
            raise ValueError(f"{path}: no *.npy frames")
        self.bgr, self.fps = bgr, 25.0

    def __len__(self):
        return len(self.files)

    def frames(self, start, stop):
        for f in self.files[start:stop]:
            yield np.ascontiguousarray(np.load(f))


class Cv2Source:
    """cv2.VideoCapture / cv2.imread: BGR frames, as the reference reads them (style_transfer.py:103-112,188)."""

    def __init__(self, path, video):
        import cv2
        self.cv2, self.path, self.video, self.bgr = cv2, path, video, True
        self.kind = "video" if video else "image"
        if video:
            cap = cv2.VideoCapture(path)
            self.n, self.fps = int(cap.get(7)), cap.get(5)
            cap.release()
        else:
            self.n, self.fps = 1, 25.0

    def __len__(self):
        return self.n

    def frames(self, start, stop):
        if not self.video:
            yield self.cv2.imread(self.path)
            return
        cap = self.cv2.VideoCapture(self.path)
        cap.set(self.cv2.CAP_PROP_POS_FRAMES, start)
        for _ in range(start, stop):
            ok, fr = cap.read()
            if not ok:
                break
            yield fr
        cap.release()


def open_source(path, video, frame_order):
    ext = os.path.splitext(path)[1].lower()
    if os.path.isdir(path):
        return DirSource(path, frame_order == "bgr")
    if ext == ".npy":
        return NpySource(path, frame_order == "bgr")
    if ext in VIDEO_EXT + IMAGE_EXT:
        try:
            import cv2  # noqa: F401
        except ImportError:
            raise SystemExit(f"{path}: reading {ext} needs cv2 (not importable here); pass frames as .npy "
                             "((N,H,W,3) uint8) or a directory of .npy frames") from None
        return Cv2Source(path, video and ext in VIDEO_EXT)
    raise SystemExit(f"{path}: unknown content type")

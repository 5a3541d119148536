"""Tiled generation (MultiDiffusion, Bar-Tal et al. 2023): the host side of a canvas stepped from overlapping windows.

Pure Python / torch CPU: where the windows sit and how their predictions are blended.  Windows sit on a Cartesian grid, so both are
separable: one list of positions and one weight table per axis.  The kernel (csrc/window_step.hip, include/fluxmi.h) multiplies the two
axes' weights in fp32 and sums weight * prediction over the covering windows; the tables made here are already normalised per canvas
position, so that sum is the blend.  Units are whatever the caller counts in (the pipeline: tokens of the packed latent, 16 px each)."""
import math
from typing import List, NamedTuple, Sequence

import torch

PROFILES = ("cosine", "uniform")


def window_positions(canvas: int, window: int, stride: int) -> List[int]:
    """p_k = min(k * stride, canvas - window) for k = 0 .. ceil((canvas - window) / stride): the last window snaps to the edge, so all windows
    are equal and the canvas is covered (its overlap with its neighbour is then larger than the others')."""
    canvas, window, stride = int(canvas), int(window), int(stride)
    if not 1 <= window <= canvas:
        raise ValueError(f"windows: window {window} outside 1..canvas ({canvas})")
    if stride < 1:
        raise ValueError(f"windows: stride {stride} < 1")
    n = -(-(canvas - window) // stride)
    return [min(k * stride, canvas - window) for k in range(n + 1)]


def window_weights(canvas: int, window: int, positions: Sequence[int], profile: str = "cosine") -> torch.Tensor:
    """fp32 [len(positions)][canvas]: the blend weight of window k at canvas position i, normalised per position (in double, then cast), zero
    outside the window.  `uniform`: every covering window counts the same.  `cosine`: 0.5 - 0.5 cos(2 pi (i + 0.5) / window) over the
    window's own positions i -- a Hann window sampled at the half positions, > 0 everywhere.  A position under one window gets exactly 1."""
    if profile not in PROFILES:
        raise ValueError(f"windows: profile {profile!r}: expected one of {PROFILES}")
    canvas, window = int(canvas), int(window)
    positions = [int(p) for p in positions]
    if not positions or any(p < 0 or p + window > canvas for p in positions):
        raise ValueError(f"windows: positions {positions} with window {window} leave the canvas ({canvas})")
    if profile == "uniform":
        prof = [1.0] * window
    else:
        prof = [0.5 - 0.5 * math.cos(2.0 * math.pi * (i + 0.5) / window) for i in range(window)]
    raw = torch.zeros((len(positions), canvas), dtype=torch.float64)
    for k, p in enumerate(positions):
        raw[k, p:p + window] = torch.tensor(prof, dtype=torch.float64)
    total = raw.sum(0)
    if bool((total <= 0).any()):
        raise ValueError(f"windows: canvas position {int((total <= 0).nonzero()[0])} is under no window (positions {positions}, window {window})")
    return (raw / total).to(torch.float32)  # (x / x == 1.0 exactly: one covering window -> 1.0f)


class WindowPlan(NamedTuple):
    """the geometry and tables of one canvas: everything fluxmi_engine_set_windows takes besides the image count"""
    Hc: int
    Wc: int
    h: int
    w: int
    row0: List[int]
    col0: List[int]
    Ny: torch.Tensor  # fp32 [ny][Hc]
    Nx: torch.Tensor  # fp32 [nx][Wc]

    @property
    def ny(self) -> int:
        return len(self.row0)

    @property
    def nx(self) -> int:
        return len(self.col0)


def plan(Hc: int, Wc: int, h: int, w: int, stride_y: int, stride_x: int, profile: str = "cosine") -> WindowPlan:
    """windows of h x w on a canvas of Hc x Wc at the given strides"""
    row0, col0 = window_positions(Hc, h, stride_y), window_positions(Wc, w, stride_x)
    return WindowPlan(int(Hc), int(Wc), int(h), int(w), row0, col0, window_weights(Hc, h, row0, profile), window_weights(Wc, w, col0, profile))

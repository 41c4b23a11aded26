"""Temporal smoothing of parsing maps on the MI355X kernels (csrc/flow_ops.hip) -- the reference's
flicker-reduction pre-pass, smooth_parsing_map.py.

    warp(x, flo)                      smooth_parsing_map.py:37-75 (same name, arguments and return pair)
    temporal_weights(window)          :140
    fuse_window(...)                  :155-167, one centre frame: warp + spatial x temporal weights + fusion + Downsample
    smooth_parsing_maps(...)          :125-168, the loop over a clip resident on the GPU (the comparison baseline)
    ParsingSmoother(raft, bisenet, window)   :114-168 as a streaming stage: uint8 frames in, smoothed maps out,
                                      device memory bounded by the window

ParsingSmoother runs RAFT (vtoonify_amd.raft, section 4.7 of DESIGN.md) and BiSeNet itself.  smooth_parsing_maps takes its
flow from `flow_fn(image1, image2) -> flow_up`: `raft_flow_fn(vtoonify_amd.raft.RAFT(...))`, or the reference's own
`raft_model(..., test_mode=True)[1]`.  GPU fp32 tensors only.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional

import numpy as np
import torch

from . import _lib
from . import kernels as K
from . import op


def _p(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def warp(x: torch.Tensor, flo: torch.Tensor):
    """warp an image/tensor (im2) back to im1 according to the optical flow: x (B,C,H,W), flo (B,2,H,W) ->
    (output * mask, mask), mask (B,C,H,W) of zeros and ones (smooth_parsing_map.py:37-75)."""
    if x.dtype != torch.float32 or flo.dtype != torch.float32:
        raise _lib.VtError("smooth.warp: fp32 tensors expected")
    K._dev_ok(x, flo)
    B, Cn, H, W = x.shape
    if tuple(flo.shape) != (B, 2, H, W):
        raise _lib.VtError("smooth.warp: flo must be (B,2,H,W)")
    out = torch.empty_like(x)
    mask = torch.empty((B, 1, H, W), dtype=torch.float32, device=x.device)
    _lib.check(_lib.lib().vt_flow_warp(_p(out), _p(mask), _p(x), _p(flo), B, Cn, H, W, K._stream(x)), "vt_flow_warp")
    return out, mask.expand(B, Cn, H, W)


def temporal_weights(window: int, device=None) -> torch.Tensor:
    """exp(-(k - window)^2 / (2 (window + 0.5)^2)), k = 0..2*window (smooth_parsing_map.py:140), shape (2w+1,)."""
    k = torch.arange(2 * window + 1, dtype=torch.float32)
    wt = torch.exp(-(k - window) ** 2 / (2 * ((window + 0.5) ** 2)))
    return wt.to(device) if device is not None else wt


def make_downsample_kernel(k=(1, 3, 3, 1), factor: int = 2) -> torch.Tensor:
    """Downsample(kernel=[1,3,3,1], factor=2).kernel (model/stylegan/model.py:53-61, make_kernel :21-29)."""
    k1 = torch.tensor(k, dtype=torch.float32)
    k2 = k1[None, :] * k1[:, None]
    return k2 / k2.sum()


def fuse_window(image1: torch.Tensor, image2: torch.Tensor, parsing: torch.Tensor, flow_up: torch.Tensor,
                wt: torch.Tensor, center_index: Optional[int] = None, sigma: float = 0.2,
                down_kernel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """smooth_parsing_map.py:155-167 for one centre frame.

    image1 (3,H,W) or (1,3,H,W): the centre frame (the reference repeats it over the window);
    image2 (2w+1,3,H,W): the window's frames; parsing (2w+1,CP,H,W): their parsing maps; flow_up (2w+1,2,H,W):
    flow from the centre frame to every window frame; wt (2w+1,) or (2w+1,1,1,1).  Returns
    down(fused_Ps): (1,CP,H/2,W/2) -- or (1,CP,H,W) when down_kernel is False."""
    for t in (image1, image2, parsing, flow_up, wt):
        if t.dtype != torch.float32:
            raise _lib.VtError("smooth.fuse_window: fp32 tensors expected")
    image1 = image1.reshape(3, *image1.shape[-2:])
    wt = wt.reshape(-1)
    K._dev_ok(image1, image2, parsing, flow_up, wt)
    wn, cp, H, W = parsing.shape
    if tuple(image2.shape) != (wn, 3, H, W) or tuple(flow_up.shape) != (wn, 2, H, W) or wt.numel() != wn or \
            tuple(image1.shape) != (3, H, W):
        raise _lib.VtError("smooth.fuse_window: window tensors disagree in shape")
    ci = wn // 2 if center_index is None else int(center_index)
    fused = torch.empty((1, cp, H, W), dtype=torch.float32, device=parsing.device)
    _lib.check(_lib.lib().vt_parsing_fuse(_p(fused), _p(image2), _p(image1), _p(parsing), _p(flow_up), _p(wt), wn, ci,
                                          cp, H, W, float(sigma), K._stream(parsing)), "vt_parsing_fuse")
    if down_kernel is False:
        return fused
    kern = make_downsample_kernel().to(parsing.device) if down_kernel is None else down_kernel
    # Downsample.forward: upfirdn2d(x, kernel, up=1, down=2, pad=(p+1)//2, p//2) with p = 4 - 2 (model.py:62-71)
    return op.upfirdn2d(fused, kern, up=1, down=2, pad=(1, 1))


def raft_flow_fn(raft_model, iters: int = 20) -> Callable[[torch.Tensor, torch.Tensor], torch.Tensor]:
    """flow_fn of smooth_parsing_maps from a RAFT module (vtoonify_amd.raft.RAFT or the reference's):
    smooth_parsing_map.py:150-151 calls `raft_model((image1+1)*255/2, (image2+1)*255/2, iters=20, test_mode=True)[1]`."""
    def fn(image1: torch.Tensor, image2: torch.Tensor) -> torch.Tensor:
        return raft_model((image1 + 1) * 255.0 / 2, (image2 + 1) * 255.0 / 2, iters=iters, test_mode=True)[1]
    return fn


def smooth_parsing_maps(Is: torch.Tensor, Ps: torch.Tensor, flow_fn: Callable[[torch.Tensor, torch.Tensor], torch.Tensor],
                        window: int, sigma: float = 0.2) -> torch.Tensor:
    """The loop of smooth_parsing_map.py:125-168 over a clip already on the GPU: Is (T,3,H,W) frames in [-1,1]
    (the reference's 2x-upsampled frames), Ps (T,CP,H,W) their parsing maps, flow_fn(image1, image2) -> flow_up
    (B,2,H,W) for B frame pairs.  Returns (T,CP,H/2,W/2)."""
    Is_ = torch.cat((Is[0:window], Is, Is[-window:]), dim=0)      # :128,135 (replicate the clip's ends)
    Ps_ = torch.cat((Ps[0:window], Ps, Ps[-window:]), dim=0)
    wt = temporal_weights(window, Is.device)
    kern = make_downsample_kernel().to(Is.device)
    out = []
    for ii in range(Is.shape[0]):
        i = ii + window
        image2 = Is_[i - window:i + window + 1].contiguous()
        image1 = Is_[i:i + 1].repeat(2 * window + 1, 1, 1, 1)
        flow_up = flow_fn(image1, image2).contiguous()
        out.append(fuse_window(Is_[i].contiguous(), image2, Ps_[i - window:i + window + 1].contiguous(), flow_up, wt,
                               window, sigma, kern))
    return torch.cat(out, dim=0)


def window_frames(ii: int, window: int, n_frames: int):
    """Frame index of each of the 2w+1 window slots of centre frame `ii` in a clip of `n_frames`: the slice
    Is_[ii : ii+2w+1] of Is_ = cat(Is[0:w], Is, Is[-w:]) (smooth_parsing_map.py:129,149).  The clip's ends are NOT
    clamped: the first centre sees frames [0..w-1, 0..w], the last [T-1-w..T-1, T-w..T-1]."""
    out = []
    for j in range(ii, ii + 2 * window + 1):
        out.append(j if j < window else (j - window if j < window + n_frames else j - 2 * window))
    return out


class _Slot:
    __slots__ = ("Is", "Ps", "feat")

    def __init__(self, Is, Ps, feat):
        self.Is, self.Ps, self.feat = Is, Ps, feat


class ParsingSmoother:
    """smooth_parsing_map.py:114-168 as a streaming stage: push uint8 frames, get the smoothed parsing maps in frame order.

        sm = ParsingSmoother(raft, bisenet, window=5)
        for chunk in source:                     # (n,H,W,3) uint8, any chunking
            for p in sm.push(chunk): ...         # each (1,19,H,W) fp32 = parse[i] of the reference
        for p in sm.flush(): ...                 # the last `window` frames (they need the clip's end)
    or `for p in sm.smooth(iterable_of_chunks)`.

    raft: vtoonify_amd.raft.RAFT or RaftEngine; bisenet: vtoonify_amd.bisenet.BiSeNet or BiSeNetEngine; bgr: the
    frames are BGR as cv2 delivers them (the reference converts, :122).

    Per frame: one vt_frame_ingest2x (Is, RAFT's input, BiSeNet's input at 2H x 2W), one BiSeNet pass, one
    RaftEngine.encode.  Per centre frame: one RaftEngine.refine over the 2w non-centre slots (the centre pair, whose
    aligned map and weight :160-162 overwrite, is not computed; vt_parsing_fuse reads neither its flow nor its frame),
    one vt_parsing_fuse, the Downsample.  Window slots that alias a frame at the clip's ends share its cached features.

    Device memory is bounded by the window, not the clip.  With S = 2H * 2W, s = S / 64 and e = bytes of RAFT's
    compute type (4 in fp32, 2 in bf16 and fp16: the GRU input rows; the feature pyramid is fp32 in every mode), a
    ring slot holds
        Is 12 S  +  Ps 76 S  +  RAFT features (1024 * 85/64 + 400 e) s          bytes,
    at most 2w+1 slots are alive (`peak_slots`), and fusing a window stages (2w+1) * 96 S bytes (frames, maps, flows)
    next to the transient activations of one BiSeNet pass and one refine of 2w pairs:
        (2w+1) * (184 S + (1360 + 400 e) s)  +  activations.
    512 x 512 after the doubling, w = 5, fp32: 11 * (48.2 + 12.1) MB = 0.66 GB whatever the clip's length.

    2H and 2W must be multiples of 8: the reference pads to RAFT's stride (InputPadder, :151-152) and then warps
    un-padded maps with the padded flow, which fails; such sizes raise VtError here."""

    def __init__(self, raft, bisenet, window: int, sigma: float = 0.2, iters: int = 20, bgr: bool = True):
        if window < 1:
            raise _lib.VtError("ParsingSmoother: window must be >= 1")
        self.raft = raft.engine() if hasattr(raft, "engine") else raft
        self.bisenet = bisenet
        self.window, self.sigma, self.iters, self.bgr = int(window), float(sigma), int(iters), bool(bgr)
        self.device = self.raft.device
        self._wt = temporal_weights(self.window, self.device)
        self._kern = make_downsample_kernel().to(self.device)
        self._slots = {}            # frame index -> _Slot
        self._arrived = 0           # frames pushed
        self._emitted = 0           # centre frames done
        self.peak_slots = 0         # largest number of ring slots alive at once
        self.encodes = self.refined_pairs = 0

    @property
    def live_slots(self) -> int:
        return len(self._slots)

    # ------------------------------------------------------------------
    @staticmethod
    def _check_size(H, W):
        if (2 * H) % 8 or (2 * W) % 8:
            raise _lib.VtError(f"ParsingSmoother: frames of {H}x{W} double to {2 * H}x{2 * W}, not multiples of 8: the "
                               "reference pads them for RAFT and then cannot warp its un-padded maps "
                               "(smooth_parsing_map.py:151-155); crop or resize the video to multiples of 4")

    def _ingest(self, frame_u8):
        Is, r_in, b_in = K.frame_ingest2x(frame_u8, self.bgr)
        Ps = self.bisenet(b_in)[0]                           # parsingpredictor(2*Is[i:i+1])[0] (:136)
        feat = self.raft.encode(r_in)
        self.encodes += 1
        return _Slot(Is, Ps.contiguous(), feat)

    def _fuse(self, ii, n_frames):
        w = self.window
        idx = window_frames(ii, w, n_frames)
        sl = [self._slots[f] for f in idx]
        others = sl[:w] + sl[w + 1:]
        flow = self.raft.refine(sl[w].feat, [s.feat for s in others], self.iters)
        self.refined_pairs += len(others)
        # vt_parsing_fuse reads neither the flow nor the frame of the centre slot (parsing_fuse_kernel: `if (j == ci)`
        # takes parsing[ci] with weight wt[ci] and continues); zeros stand there all the same
        flow_all = torch.cat([flow[:w], flow.new_zeros((1,) + tuple(flow.shape[1:])), flow[w:]], 0)
        image2 = torch.cat([s.Is for s in sl], 0)
        parsing = torch.cat([s.Ps for s in sl], 0)
        out = fuse_window(sl[w].Is, image2, parsing, flow_all, self._wt, w, self.sigma, self._kern)
        for f in [f for f in self._slots if f < ii + 1 - w]:          # no later centre reaches back further
            del self._slots[f]
        return out

    @torch.no_grad()
    def push(self, frames_uint8: torch.Tensor):
        """(n,H,W,3) or (H,W,3) uint8 frames (a CPU tensor is copied to the device) -> the list of maps that became
        computable, each (1,19,H,W) fp32 on the device, in frame order."""
        if frames_uint8.ndim == 3:
            frames_uint8 = frames_uint8[None]
        if frames_uint8.dtype != torch.uint8 or frames_uint8.ndim != 4 or frames_uint8.shape[-1] != 3:
            raise _lib.VtError("ParsingSmoother.push: frames must be (n,H,W,3) uint8")
        self._check_size(int(frames_uint8.shape[1]), int(frames_uint8.shape[2]))
        out = []
        for k in range(frames_uint8.shape[0]):
            self._slots[self._arrived] = self._ingest(frames_uint8[k:k + 1].to(self.device).contiguous())
            self._arrived += 1
            self.peak_slots = max(self.peak_slots, len(self._slots))
            if self._arrived - 1 - self.window >= self._emitted:      # centre t - w: its last frame has just arrived
                out.append(self._fuse(self._emitted, self._arrived + self.window))   # (any n_frames beyond the window)
                self._emitted += 1
        return out

    @torch.no_grad()
    def flush(self):
        """End of the clip: the maps of the remaining frames (the last `window`), whose windows replicate the clip's
        end as the reference does.  The smoother is empty afterwards and can take another clip."""
        T = self._arrived
        if 0 < T < self.window:
            self.reset()
            raise _lib.VtError(f"ParsingSmoother: a clip of {T} frames is shorter than the window ({self.window}); the "
                               "reference's end replication Is[0:w], Is[-w:] needs at least w frames")
        out = []
        while self._emitted < T:
            out.append(self._fuse(self._emitted, T))
            self._emitted += 1
        self.reset()
        return out

    @torch.no_grad()
    def smooth_shard(self, frames, n_frames: int, start: int, stop: int):
        """The maps of centre frames [start, stop) of a clip of `n_frames`, for a rank that owns that shard: `frames`
        yields the clip's uint8 frames (H,W,3) from index max(0, start - w) on, in order, and is read up to
        min(n_frames, stop + w) -- w frames of context on either side, the neighbour shard's real frames; only the
        clip's own ends replicate.  Yields what the one-pass stage yields for those frames, bit for bit (every frame is
        ingested alone and every centre refines 2w pairs, whatever the shard)."""
        w = self.window
        if not (0 <= start <= stop <= n_frames) or n_frames < w:
            raise _lib.VtError(f"ParsingSmoother.smooth_shard: bad shard [{start},{stop}) of {n_frames} frames (window {w})")
        self.reset()
        it = iter(frames)
        nxt = max(0, start - w)
        for ii in range(start, stop):
            last = max(window_frames(ii, w, n_frames))
            while nxt <= last:
                fr = next(it)
                fr = fr if isinstance(fr, torch.Tensor) else torch.from_numpy(np.array(fr))      # (a memmap row: copy)
                if fr.ndim == 3:
                    fr = fr[None]
                if fr.dtype != torch.uint8 or fr.ndim != 4 or fr.shape[0] != 1 or fr.shape[-1] != 3:
                    raise _lib.VtError("ParsingSmoother.smooth_shard: frames must be (H,W,3) uint8")
                self._check_size(int(fr.shape[1]), int(fr.shape[2]))
                self._slots[nxt] = self._ingest(fr.to(self.device).contiguous())
                nxt += 1
                self.peak_slots = max(self.peak_slots, len(self._slots))
            yield self._fuse(ii, n_frames)
        self.reset()

    def reset(self):
        self._slots.clear()
        self._arrived = self._emitted = 0

    def smooth(self, chunks):
        """Iterator form: chunks of uint8 frames in, maps out in frame order (flushes at the end)."""
        for c in chunks:
            yield from self.push(c)
        yield from self.flush()

"""Executable definition of the stabiliser's inpainting (include/rsdsfm_stabilize_inpaint.h): the pixels of a frame that no frame of the clip
saw, from an integer pull-push pyramid of what surrounds them -- the dense rectifier's stage A (tests/rectify_dense_spec_numpy.py), for
bytes.  The reference has no counterpart (main.cc:380-523 solves pairs one by one and renders nothing of this kind); this file is the
definition and the kernels (csrc/stabilize_inpaint_kernels.hip) and host functions (csrc/stabilize_inpaint_host.hip) reproduce it bit for bit.
The call is generic: any image of 1 or 3 channels and any validity mask.

Non-negative integers only.

level 0     v = byte << 8 per channel; a cell is valid iff its mask byte != 0 (one validity for all channels).
pull        level l (h x w) -> level l + 1 (ceil(h / 2) x ceil(w / 2)), down to 1 x 1.  A cell has up to four children; children outside the
            level are absent.  With n valid children v = (sum of the valid children + (n >> 1)) // n per channel and the cell is valid; with
            n = 0 it is invalid.
push        from coarse to fine; the 1 x 1 level is complete if it is valid.  An invalid cell (y, x) of level l takes from the complete level
            l + 1 (hc x wc): yn = y >> 1, yf = clamp(yn + (1 if y odd else -1), 0, hc - 1), xn and xf alike,
            v = (9 c[yn, xn] + 3 c[yn, xf] + 3 c[yf, xn] + c[yf, xf] + 8) >> 4 -- the dense rectifier's sample position ((x + 1/2) / 2 - 1/2,
            replicate border) with exact weights.  A valid cell keeps its value.
inpaint     in place: an empty pixel of level 0 gets (v + 128) >> 8 per channel and, in the source plane when one is passed, SOURCE_INPAINTED;
            a set pixel keeps its bytes; the mask is only read.  Returns the number of pixels written.  Without any set pixel the 1 x 1 level
            is invalid: nothing is written, 0 is returned.

Every level value is <= 255 << 8 = 65280 (a mean and a convex combination of such values): 16 bits per channel, no clamp anywhere.

Not here: exemplar, patch or diffusion inpainting, temporal consistency of the invented pixels, the clip's last frame.
"""
import numpy as np

SOURCE_INPAINTED = 255  # the source byte of an inpainted pixel; the clip's candidates have ids <= 33


def pull(v, valid):
    """one level up: v (h, w, CH) int64 with 0 in its invalid cells, valid (h, w) bool -> (v, valid) of ceil(h / 2) x ceil(w / 2)"""
    h, w = valid.shape
    hn, wn = (h + 1) // 2, (w + 1) // 2
    vp = np.zeros((2 * hn, 2 * wn, v.shape[2]), dtype=np.int64)
    mp = np.zeros((2 * hn, 2 * wn), dtype=np.int64)
    vp[:h, :w] = v
    mp[:h, :w] = valid
    s = vp[0::2, 0::2] + vp[0::2, 1::2] + vp[1::2, 0::2] + vp[1::2, 1::2]
    n = mp[0::2, 0::2] + mp[0::2, 1::2] + mp[1::2, 0::2] + mp[1::2, 1::2]
    out = (s + (n >> 1)[..., None]) // np.maximum(n, 1)[..., None]
    return np.where((n > 0)[..., None], out, 0), n > 0


def push(v, valid, coarse):
    """level (h, w) completed from the complete coarser level: the invalid cells take the sample, the valid ones keep their value"""
    h, w = valid.shape
    hc, wc = coarse.shape[:2]
    y, x = np.arange(h), np.arange(w)
    yn, xn = y >> 1, x >> 1
    yf = np.clip(yn + np.where(y & 1, 1, -1), 0, hc - 1)
    xf = np.clip(xn + np.where(x & 1, 1, -1), 0, wc - 1)
    c = lambda yy, xx: coarse[yy][:, xx]
    s = (9 * c(yn, xn) + 3 * c(yn, xf) + 3 * c(yf, xn) + c(yf, xf) + 8) >> 4
    return np.where(valid[..., None], v, s)


def pyramid(image, mask):
    """-> (levels, valids): level 0 .. the 1 x 1 level as pulled, each (h, w, CH) int64 / (h, w) bool"""
    img = np.asarray(image)
    valid = np.asarray(mask) != 0
    v = img.reshape(valid.shape + (-1,)).astype(np.int64) << 8
    levels, valids = [np.where(valid[..., None], v, 0)], [valid]
    while levels[-1].shape[0] > 1 or levels[-1].shape[1] > 1:
        v, valid = pull(levels[-1], valids[-1])
        levels.append(v)
        valids.append(valid)
    return levels, valids


def inpaint(image, mask, source=None):
    """in place on image ((rows, cols) or (rows, cols, 3) uint8) and source ((rows, cols) uint8 or None); mask (rows, cols) uint8 is only
    read.  Returns the number of pixels written."""
    assert image.dtype == np.uint8 and image.shape[:2] == np.asarray(mask).shape and (image.ndim == 2 or image.shape[2] in (1, 3))
    levels, valids = pyramid(image, mask)
    if not valids[-1][0, 0]:
        return 0
    full = levels[-1]
    for l in range(len(levels) - 2, -1, -1):
        full = push(levels[l], valids[l], full)
    assert full.min() >= 0 and full.max() <= 65280
    empty = ~valids[0]
    out = ((full + 128) >> 8).astype(np.uint8).reshape(image.shape)
    image[empty] = out[empty]
    if source is not None:
        source[empty] = SOURCE_INPAINTED
    return int(empty.sum())

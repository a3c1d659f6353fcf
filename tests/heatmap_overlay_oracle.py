"""float64 numpy restatement of the heat-map overlay's drawing rule (csrc/render.hip: render_heatmap_kernel).
The kernel must agree with it bit for bit.

For output pixel (y, x) of a view with image luma [H, W] uint8 and heat-maps hm [P, Hh, Wh] float32:

    sy = double(y Hh) / double(H)                       the arg-max convention: pixel = cell * H / Hh, not pixel centres
    sx = double(xs Wh) / double(W),  xs = W - x for a view the network saw mirrored, else x
    i0 = min(floor(sy), Hh - 1), i1 = min(i0 + 1, Hh - 1), fy = sy - floor(sy) if floor(sy) <= Hh - 1 else 0     (columns alike)
    per selected plane, taps as float64, a non-finite tap reads as 0, no fused multiply-add:
        top = (1 - fx) h00 + fx h01;  bot = (1 - fx) h10 + fx h11;  v = (1 - fy) top + fy bot;  a = min(max(gain v, 0), 1)
    the winner is the selected plane of largest a, the earliest of equals
    out[ch] = floor((1 - a) g + a C[ch] + 0.5)
"""
import numpy as np


def _taps(s, n):
    fl = np.floor(s)
    inside = fl <= n - 1
    i0 = np.where(inside, fl, n - 1).astype(np.int64)
    f = np.where(inside, s - fl, 0.0)
    return i0, np.minimum(i0 + 1, n - 1), f


def alpha(hm, sel, H, W, flip, gain=1.0):
    """[n, H, W] float64: the clamped sample a of every selected plane at every pixel."""
    hm = np.asarray(hm, dtype=np.float32)
    Hh, Wh = hm.shape[1:]
    y = np.arange(H, dtype=np.int64)
    x = np.arange(W, dtype=np.int64)
    xs = W - x if flip else x
    i0, i1, fy = _taps((y * Hh).astype(np.float64) / np.float64(H), Hh)
    j0, j1, fx = _taps((xs * Wh).astype(np.float64) / np.float64(W), Wh)
    fy, fx = fy[:, None], fx[None, :]
    out = np.zeros((len(sel), H, W), dtype=np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k, p in enumerate(sel):
            h = hm[int(p)].astype(np.float64)
            h = np.where(np.isfinite(h), h, 0.0)
            h00, h01, h10, h11 = h[np.ix_(i0, j0)], h[np.ix_(i0, j1)], h[np.ix_(i1, j0)], h[np.ix_(i1, j1)]
            top = (1.0 - fx) * h00 + fx * h01
            bot = (1.0 - fx) * h10 + fx * h11
            v = (1.0 - fy) * top + fy * bot
            out[k] = np.minimum(np.maximum(np.float64(gain) * v, 0.0), 1.0)
    return out


def overlay_view(luma, hm, sel, colors, flip, gain=1.0):
    """luma [H, W] uint8, hm [P, Hh, Wh] float32, sel the selected planes in order, colors one RGB triple per selected plane
    -> [H, W, 3] uint8."""
    luma = np.asarray(luma, dtype=np.uint8)
    H, W = luma.shape
    g = luma.astype(np.float64)
    best = np.zeros((H, W), dtype=np.float64)
    colour = np.zeros((H, W, 3), dtype=np.float64)
    if len(sel):
        a = alpha(hm, sel, H, W, flip, gain)
        rgb = np.asarray(colors, dtype=np.float64).reshape(len(sel), 3)
        for k in range(len(sel)):
            win = a[k] > best   # strict: a tie stays with the earlier plane
            best = np.where(win, a[k], best)
            colour = np.where(win[..., None], rgb[k], colour)
    out = np.floor((1.0 - best)[..., None] * g[..., None] + best[..., None] * colour + 0.5)
    return out.astype(np.uint8)


def overlay_grid(luma, hm, sels, colors, flips, gain=1.0, cols=None, fill=0):
    """luma [S, H, W], hm [S, P, Hh, Wh], per-view tables -> [ceil(S / cols) H, cols W, 3] uint8, view s at cell (s // cols, s % cols);
    cells past the last view hold `fill`."""
    S, H, W = np.asarray(luma).shape
    cols = S if cols is None else cols
    rows = -(-S // cols)
    out = np.full((rows * H, cols * W, 3), fill, dtype=np.uint8)
    for s in range(S):
        r, c = divmod(s, cols)
        out[r * H:(r + 1) * H, c * W:(c + 1) * W] = overlay_view(luma[s], hm[s], sels[s], colors[s], flips[s], gain)
    return out

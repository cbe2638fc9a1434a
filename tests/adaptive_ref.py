"""numpy restatement of adaptive sampling (csrc/adaptive.hip): the per-tile error of two half films, the active list, and the
pass schedule of mcpt_render_adaptive.  Films are (h, w, 4) float arrays of {sum rgb, count} records."""
from __future__ import annotations

import numpy as np


def display(film: np.ndarray) -> np.ndarray:
    """sqrt(clamp(mean, 0, 1)) per channel, what mcpt_tonemap shows before the x255.99; a count of 0 reads as a mean of 0."""
    f = np.asarray(film, np.float64)
    n = f[..., 3:]
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(n > 0, f[..., :3] / np.where(n > 0, n, 1), 0.0)
    return np.sqrt(np.clip(np.nan_to_num(m, nan=0.0), 0.0, 1.0))


def pixel_error(h: np.ndarray, o: np.ndarray) -> np.ndarray:
    """e_p = sum over rgb of |sqrt(clamp(H/nH)) - sqrt(clamp(O/nO))|, (h, w)."""
    return np.abs(display(h) - display(o)).sum(axis=-1)


def tiles_shape(height: int, width: int):
    return (height + 7) // 8, (width + 7) // 8


def tile_error(h: np.ndarray, o: np.ndarray):
    """(E_t, c_t), each (tiles_y, tiles_x): the max of e_p over the tile's in-image pixels, and nH + nO of the tile's first pixel."""
    H, W = h.shape[:2]
    ty, tx = tiles_shape(H, W)
    e = np.zeros((ty * 8, tx * 8))
    e[:H, :W] = pixel_error(h, o)
    E = e.reshape(ty, 8, tx, 8).max(axis=(1, 3))
    c = (np.asarray(h, np.float64)[..., 3] + np.asarray(o, np.float64)[..., 3])[::8, ::8]
    return E, c


def active_list(E: np.ndarray, c: np.ndarray, threshold: float, max_spp: int) -> np.ndarray:
    """Row-major numbers of the tiles with E_t >= threshold and c_t < max_spp, ascending."""
    act = (E >= threshold) & (c < max_spp)
    return np.flatnonzero(act.reshape(-1)).astype(np.uint32)


def schedule(min_spp: int, max_spp: int):
    """The passes a tile that stays active goes through: [(c, n, nh)] -- samples [c, c + n) of the pass (relative to first_sample), the first
    nh of them into H, the rest into O."""
    assert min_spp >= 2 and min_spp % 2 == 0 and max_spp >= min_spp
    out = [(0, min_spp, min_spp // 2)]
    c = min_spp
    while c < max_spp:
        n = min(c, max_spp - c)
        out.append((c, n, n // 2))
        c += n
    return out


def allowed_counts(min_spp: int, max_spp: int):
    """The sample counts a tile can end with: min * 2^k below max, and max."""
    return sorted({c + n for c, n, _ in schedule(min_spp, max_spp)})


def pass_ranges(min_spp: int, max_spp: int, count: int):
    """The H and O sample ranges [(start, n)] (relative to first_sample) a tile that ended with `count` samples received."""
    hs, os_ = [], []
    for c, n, nh in schedule(min_spp, max_spp):
        if c >= count:
            break
        if nh:
            hs.append((c, nh))
        os_.append((c + nh, n - nh))
    return hs, os_


def display_rmse(film: np.ndarray, ref: np.ndarray) -> float:
    """RMSE of sqrt(clamp(mean, 0, 1)) against a reference film, over all pixels and channels."""
    return float(np.sqrt(np.mean((display(film) - display(ref)) ** 2)))

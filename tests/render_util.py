"""Plain NumPy restatement of the rgb_array raster rule of ``mapf_render`` (include/mapf_step.h), for the tests.

Deliberately obvious: the rule's steps in its order, over whole-frame index arrays (``y``, ``x``) and the cell slices
the goal, disc and window steps touch.  Integer arithmetic throughout, so frames compare with ``np.array_equal``.
"""

from __future__ import annotations

import numpy as np

# the reference's 16 agent colours in its order (CSS RGB)
PALETTE_HEX = (
    ("red", 0xFF0000), ("blue", 0x0000FF), ("green", 0x008000), ("purple", 0x800080), ("orange", 0xFFA500),
    ("cyan", 0x00FFFF), ("magenta", 0xFF00FF), ("yellow", 0xFFFF00), ("brown", 0xA52A2A), ("pink", 0xFFC0CB),
    ("olive", 0x808000), ("teal", 0x008080), ("navy", 0x000080), ("gold", 0xFFD700), ("lime", 0x00FF00),
    ("gray", 0x808080),
)
PALETTE = np.array([[(v >> 16) & 255, (v >> 8) & 255, v & 255] for _, v in PALETTE_HEX], dtype=np.int64)

WHITE, BLACK, GRAY = (255, 255, 255), (0, 0, 0), (128, 128, 128)


def palette(a: int) -> np.ndarray:
    return PALETTE[a % 16]


def blend(d, s, alpha: int):
    """(s * alpha + d * (255 - alpha) + 127) // 255 per channel."""
    d = np.asarray(d, dtype=np.int64)
    s = np.asarray(s, dtype=np.int64)
    return (s * alpha + d * (255 - alpha) + 127) // 255


def cell_offsets(c: int):
    """dx, dy [c, c] (row = y offset in the cell, column = x offset) of the pixels of a cell, in half pixels from its
    centre: dx = 2x + 1 - c(2j + 1) with x = j*c + xm."""
    ym, xm = np.indices((c, c))
    return 2 * xm + 1 - c, 2 * ym + 1 - c


def disc_mask(c: int) -> np.ndarray:
    dx, dy = cell_offsets(c)
    return 25 * (dx * dx + dy * dy) <= 9 * c * c


def diamond_mask(c: int) -> np.ndarray:
    dx, dy = cell_offsets(c)
    return np.abs(dx) + np.abs(dy) <= c


def line_mask(c: int) -> np.ndarray:
    ym, xm = np.indices((c, c))
    return (ym == 0) | (xm == 0)


def render_frame(grid, positions, goals, c: int, sensor_range=None) -> np.ndarray:
    """uint8 [H*c, W*c, 3] frame of one env.  positions / goals: [N, 2] (row, col); sensor_range None = no windows (the
    single-agent env)."""
    grid = np.asarray(grid)
    positions = np.asarray(positions).reshape(-1, 2)
    goals = np.asarray(goals).reshape(-1, 2)
    H, W = grid.shape
    y, x = np.indices((H * c, W * c))
    i, j = y // c, x // c
    # 1. base colour
    img = np.where((grid[i, j] != 0)[..., None], np.array(BLACK), np.array(WHITE)).astype(np.int64)
    # 2. grid lines, obstacle cells included
    img[(y % c == 0) | (x % c == 0)] = GRAY

    def cell(r, q):
        return img[r * c:(r + 1) * c, q * c:(q + 1) * c]  # a view: writes go to img

    # 3. goal diamonds
    dia = diamond_mask(c)
    for g, (gr, gq) in enumerate(goals):
        if 0 <= gr < H and 0 <= gq < W:
            v = cell(gr, gq)
            v[dia] = blend(v[dia], palette(g), 128)
    # 4. agents in order: disc, then sensor window
    disc = disc_mask(c)
    for a, (r, q) in enumerate(positions):
        if 0 <= r < H and 0 <= q < W:
            cell(r, q)[disc] = palette(a)
        if sensor_range is not None:
            r0, r1 = max(r - sensor_range, 0), min(r + sensor_range, H - 1)
            q0, q1 = max(q - sensor_range, 0), min(q + sensor_range, W - 1)
            if r0 <= r1 and q0 <= q1:
                win = img[r0 * c:(r1 + 1) * c, q0 * c:(q1 + 1) * c]
                win[...] = blend(win, palette(a), 51)
    return img.astype(np.uint8)


def render_envs(grids, positions, goals, env_ids, c: int, sensor_range=None) -> np.ndarray:
    """Frames [K, H*c, W*c, 3] of envs env_ids; grids [H, W] (shared) or [B, H, W], positions / goals [B, N, 2] as
    ``get_state()`` returns them."""
    grids = np.asarray(grids)
    out = []
    for b in env_ids:
        g = grids if grids.ndim == 2 else grids[b if grids.shape[0] > 1 else 0]
        out.append(render_frame(g, positions[b], goals[b], c, sensor_range))
    return np.stack(out)

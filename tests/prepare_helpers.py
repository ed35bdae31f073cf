"""Shared inputs of the prepare tests (host and GPU): synthetic identities of any size, hand-built parsing columns that
reach the branches a natural scene does not, and a scalar restatement of the torso steps (one Python loop per column,
nothing shared with instag_amd.prepare but the darkening factors and the blur weights, which are restated here)."""
import numpy as np

HEAD, NECK, TORSO, BACKGROUND = (0, 0, 255), (0, 255, 0), (255, 0, 0), (255, 255, 255)


def scene(F, H, W, seed):
    """ori, parsing [F,H,W,3] uint8: a head ellipse, a neck bar and a torso block, jittered per frame, sized to the
    image; noise colours."""
    rng = np.random.default_rng(seed)
    ori = rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    parsing = np.full((F, H, W, 3), 255, dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    for f in range(F):
        cy, cx = int(0.3 * H) + rng.integers(-3, 4), W // 2 + rng.integers(-4, 5)
        ry, rx = int(0.15 * H) + rng.integers(-1, 2), max(3, int(0.2 * W)) + rng.integers(-1, 2)
        head = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        bottom = cy + ry
        nw = max(1, rx // 2) + rng.integers(0, 3)
        neck = (yy >= bottom - 2) & (yy < bottom + 5 + rng.integers(0, 3)) & (np.abs(xx - cx) <= nw) & ~head
        top = neck.nonzero()[0].max() + 1
        torso = (yy >= top - (np.abs(xx - cx) <= nw + 3) * 2) & (yy < H - rng.integers(0, 3)) \
            & (np.abs(xx - cx) <= int(0.3 * W) + rng.integers(0, 3)) & ~head & ~neck
        parsing[f][head], parsing[f][neck], parsing[f][torso] = HEAD, NECK, TORSO
    return ori, parsing


def special_parsing(H, W):
    """[3,H,W,3] hand-built parsing maps (W >= 9, H >= 64); the columns not named are background.

    frame 0  column 1: torso rows 0..5 under head at row H-1   -> the torso paint starts at row 0 and wraps to the last rows
             column 2: torso rows 0..5, row H-1 background      -> does not qualify
             column 4: neck at row 0, head at row H-1            -> dilated rows 0..3: c - 1 = 3 < 4, the paint wraps
             column 7: torso rows 30..40 under background        -> does not qualify
    frame 1  column 1: neck at row H-1, head at row H-5          -> dilated rows H-4..H-1: c - 1 = 3 < 4
             column 4: head 10..21, neck 22, head 23..25, torso 26..40 -> both paints qualify and overlap: rows 18..23
                       take the neck paint, rows 24..26 keep the torso paint
             column 5: head 10..25, torso 26..40                  -> the torso paint alone, next to column 4's blur
    frame 2  torso rows 30..40 in columns 2..6, nothing above     -> no column qualifies for either paint"""
    p = np.full((3, H, W, 3), 255, dtype=np.uint8)
    p[0, 0:6, 1], p[0, H - 1, 1] = TORSO, HEAD
    p[0, 0:6, 2] = TORSO
    p[0, 0, 4], p[0, H - 1, 4] = NECK, HEAD
    p[0, 30:41, 7] = TORSO
    p[1, H - 1, 1], p[1, H - 5, 1] = NECK, HEAD
    p[1, 10:26, 4], p[1, 22, 4], p[1, 26:41, 4] = HEAD, NECK, TORSO
    p[1, 10:26, 5], p[1, 26:41, 5] = HEAD, TORSO
    p[2, 30:41, 2:7] = TORSO
    return p


def special_frames(H, W, seed=5):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8), special_parsing(H, W), \
        rng.integers(0, 256, (H, W, 3), dtype=np.uint8)


def _is(px, colour):
    return tuple(int(v) for v in px) == colour


def naive_frame(ori, par, bc):
    """One frame, column by column in scalar Python -> gt [H,W,3], torso [H,W,4], painted3, painted4 [H,W] bool."""
    H, W = par.shape[:2]
    scaler = 0.98 ** np.arange(53)                       # the factors as the reference forms them
    q = (48, 53, 54, 53, 48)
    gt = ori.copy()
    for y in range(H):
        for x in range(W):
            if _is(par[y, x], BACKGROUND):
                gt[y, x] = bc[y, x]
    t = gt.copy()
    for y in range(H):
        for x in range(W):
            if _is(par[y, x], HEAD):
                t[y, x] = bc[y, x]
    p3, p4 = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    dn = np.zeros((H, W), dtype=bool)
    for x in range(W):
        rows = [y for y in range(H) if _is(par[y, x], TORSO)]
        if rows and _is(par[rows[0] - 1, x], HEAD):      # (a negative index wraps, as in the reference)
            y = rows[0]
            for k in range(9):
                t[y - k, x] = [int(float(v) * scaler[k]) for v in gt[y, x]]
                p3[y - k, x] = True
    for x in range(W):
        neck = [y for y in range(H) if _is(par[y, x], NECK)]
        for y in range(H):
            dn[y, x] = any(abs(y - n) <= 3 for n in neck)
        rows = [y for y in range(H) if dn[y, x]]
        if rows and _is(par[rows[0] - 1, x], HEAD):
            y = rows[0] + min(len(rows) - 1, 4)
            for k in range(53):
                t[y - k, x] = [int(float(v) * scaler[k]) for v in gt[y, x]]
                p4[y - k, x] = True
    pre = t.astype(np.int64)

    def at(y, x):
        y, x = abs(y), abs(x)
        return pre[2 * H - 2 - y if y >= H else y, 2 * W - 2 - x if x >= W else x]

    for y, x in zip(*np.nonzero(p4)):
        s = sum(q[dy + 2] * q[dx + 2] * at(y + dy, x + dx) for dy in range(-2, 3) for dx in range(-2, 3))
        t[y, x] = (s + 32768) >> 16
    torso = np.zeros((H, W, 4), dtype=np.uint8)
    for y in range(H):
        for x in range(W):
            if dn[y, x] or p3[y, x] or p4[y, x] or _is(par[y, x], TORSO):
                torso[y, x, :3], torso[y, x, 3] = t[y, x], 255
    return gt, torso, p3, p4

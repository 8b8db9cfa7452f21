"""Inputs and plain numpy references of the keyframe image front end's seam suite (csrc/img_kernels.h: k_pyr_fast, k_row_tables,
k_row_count + k_row_compact, k_dilate5 / k_glare_mask, k_nonmax_scores, k_candidates, k_minipatch).

tests/test_img_seams_cpu.py checks the CPU oracle against the references below and asserts what the inputs promise;
tests/test_img_seams_gpu.py runs the same inputs on the device.  Importable without a GPU.  Run as a script
(`python img_seam_cases.py OUT.npz`) it runs the row-table cases on the device and saves their tables: the child process of the
MCP_IMG_ROW_TABLES=0 test.

The references follow the definitions, not the kernels: no rotate-and-AND, no min/max tree, no LUT.  Positions are (x, y)."""
import os
import sys

import numpy as np

LEVELS = 4
FIXED_T = (10, 15, 15, 10)                 # thresholds of an adaptive=False handle, per level
MIN_T, MAX_T = 5, 30                       # range of the adaptive threshold
# the 16 pixels of the radius-3 circle, counter-clockwise from straight below (x, y)
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3))
MAXSSD = 9999


# ------------------------------------------------------------------------------------------------ plain references
def half_sample(img, pavgb=False):
    """(h >> 1, w >> 1): truncating mean of each 2x2 block, or the cascaded round-half-up averages of the pavgb path."""
    oh, ow = img.shape[0] >> 1, img.shape[1] >> 1
    I = img.astype(np.int64)
    a, b = I[0:2 * oh:2, 0:2 * ow:2], I[0:2 * oh:2, 1:2 * ow:2]
    c, d = I[1:2 * oh:2, 0:2 * ow:2], I[1:2 * oh:2, 1:2 * ow:2]
    if pavgb:
        return ((((a + c + 1) >> 1) + ((b + d + 1) >> 1) + 1) >> 1).astype(np.uint8)
    return ((a + b + c + d) // 4).astype(np.uint8)


def pyramid(img, pavgb=False):
    out = [np.ascontiguousarray(img, dtype=np.uint8)]
    for _ in range(1, LEVELS):
        out.append(half_sample(out[-1], pavgb))
    return out


def segment_test(ring, c, b):
    """FAST-10: for one of the 16 starts, are 10 consecutive ring pixels all > c + b, or all < c - b?  ring: (16, ...), c and b
    broadcast against ring[0]."""
    out = np.zeros(np.broadcast(ring[0], c, b).shape, dtype=bool)
    for flags in (ring > c + b, ring < c - b):
        for s in range(16):
            ok = np.ones(out.shape, dtype=bool)
            for j in range(10):
                ok &= flags[(s + j) % 16]
            out |= ok
    return out


def fast_corners(img, b):
    """Every pixel with 3 <= x < w - 3, 3 <= y < h - 3 that passes the segment test at threshold b, in raster order."""
    h, w = img.shape
    if h < 7 or w < 7:
        return np.zeros((0, 2), dtype=np.int32)
    I = img.astype(np.int32)
    ring = np.stack([I[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in RING])
    ys, xs = np.nonzero(segment_test(ring, I[3:h - 3, 3:w - 3], b))
    return np.stack([xs + 3, ys + 3], axis=1).astype(np.int32)


def fast_scores(img, pts):
    """The largest b in 0 .. 254 at which each of pts still passes the segment test (-1: none)."""
    pts = np.asarray(pts).reshape(-1, 2)
    if len(pts) == 0:
        return np.zeros(0, dtype=np.int64)
    I = img.astype(np.int32)
    ring = np.stack([I[pts[:, 1] + dy, pts[:, 0] + dx] for dx, dy in RING])[:, :, None]
    c = I[pts[:, 1], pts[:, 0]][:, None]
    bs = np.arange(255)[None, :]
    passes = segment_test(ring, c, bs)
    return (passes * (bs + 1)).max(axis=1) - 1


def dilate5(img):
    """One dilation by the 5x5 ellipse (rows of 1, 5, 5, 5, 1 pixels); outside the image counts as nothing."""
    h, w = img.shape
    P = np.zeros((h + 4, w + 4), dtype=np.uint8)
    P[2:h + 2, 2:w + 2] = img
    out = np.zeros((h, w), dtype=np.uint8)
    for dy in range(-2, 3):
        for dx in range(-2, 3):
            if abs(dy) == 2 and dx != 0:
                continue
            out = np.maximum(out, P[2 + dy:h + 2 + dy, 2 + dx:w + 2 + dx])
    return out


def glare(img):
    """True where the five-fold dilation of img exceeds 245: the pixels glare masking removes."""
    a = np.ascontiguousarray(img, dtype=np.uint8)
    for _ in range(5):
        a = dilate5(a)
    return a > 245


def row_lut(corners, h):
    return np.searchsorted(np.asarray(corners).reshape(-1, 2)[:, 1], np.arange(h)).astype(np.int32)


def minipatch_ref(simg, dimg, corners, src_pos, dst_pos, rng):
    """MiniPatch by brute force: the 9x9 patch of simg at src_pos against dimg at every corner inside the (2 rng + 1)^2 window around
    dst_pos, in list order, first smallest SSD wins; a corner whose patch leaves the image counts MAXSSD + 1.  (pos, found, ssd)."""
    sh, sw = simg.shape
    dh, dw = dimg.shape
    S, D = simg.astype(np.int64), dimg.astype(np.int64)
    n = len(src_pos)
    pos = np.array(dst_pos, dtype=np.int32).reshape(n, 2)
    found = np.zeros(n, dtype=bool)
    ssd = np.full(n, MAXSSD + 1, dtype=np.int32)
    for i in range(n):
        sx, sy = (int(v) for v in src_pos[i])
        dx, dy = (int(v) for v in dst_pos[i])
        if not (4 <= sx < sw - 4 and 4 <= sy < sh - 4):
            continue
        patch = S[sy - 4:sy + 5, sx - 4:sx + 5]
        best, bp = MAXSSD + 1, None
        for cx, cy in corners:
            if abs(int(cx) - dx) > rng or abs(int(cy) - dy) > rng:
                continue
            if 4 <= cx < dw - 4 and 4 <= cy < dh - 4:
                v = int(((D[cy - 4:cy + 5, cx - 4:cx + 5] - patch) ** 2).sum())
            else:
                v = MAXSSD + 1
            if v < best:
                best, bp = v, (cx, cy)
        ssd[i] = best
        if best < MAXSSD:
            pos[i] = bp
            found[i] = True
    return pos, found, ssd


# ------------------------------------------------------------------------------------------------ images
def noise(w, h, seed, hi=256):
    return np.random.default_rng(seed).integers(0, hi, size=(h, w), dtype=np.uint8)


def multi_octave(w, h, seed, amp=105):
    """A low-contrast image: random fields upsampled by 1, 2, 4 and 8, summed, scaled to `amp` grey levels around 128."""
    rng = np.random.default_rng(seed)
    f = np.zeros((h, w))
    for k in (1, 2, 4, 8):
        g = rng.random(((h + k - 1) // k, (w + k - 1) // k))
        f += np.kron(g, np.ones((k, k)))[:h, :w]
    f = (f - f.min()) / (f.max() - f.min())
    return np.floor(128 - amp / 2.0 + amp * f).astype(np.uint8)


def subset_masks(w, h, corners):
    """The mask trick: level-0 mask 255 exactly on `corners` and 0 elsewhere, no mask above.  On an adaptive handle the threshold comes
    from all detected corners, so a subset of the unmasked run's corners is left exactly, at the same threshold."""
    m = np.zeros((h, w), dtype=np.uint8)
    c = np.asarray(corners).reshape(-1, 2)
    m[c[:, 1], c[:, 0]] = 255
    return [m, None, None, None]


def level_masks(w, h, seed):
    """Caller masks of every level but 2: a masked band, a masked block and scattered 254s ("< 255" is masked out too)."""
    rng = np.random.default_rng(seed)
    out = []
    for l in range(LEVELS):
        hl, wl = h >> l, w >> l
        m = np.full((hl, wl), 255, dtype=np.uint8)
        m[:hl // 5, :] = 0
        m[hl // 2:hl // 2 + 3, wl // 2:] = 0
        m[rng.integers(0, hl, 40), rng.integers(0, wl, 40)] = 254
        out.append(None if l == 2 else m)
    return out


# ------------------------------------------------------------------------------------------------ 1. stamps
STAMP_C = 120
ORIGINS = (13, 14, 15, 16, 17, 18)         # centres at origin + 16 i: columns and rows 61 .. 66 modulo 64 (and T - 3 .. T + 2 modulo 32, 16)


def put_stamp(img, cx, cy, c, start, length, ring_value):
    img[cy, cx] = c
    for j in range(length):
        dx, dy = RING[(start + j) % 16]
        img[cy + dy, cx + dx] = ring_value


def stamp_sheet(params, size, origin, pitch, per_row):
    """params: (start, length, sign, d) per stamp, on a lattice of `pitch` from `origin`; background and centres STAMP_C.
    Returns (sheet, centres)."""
    img = np.full((size, size), STAMP_C, dtype=np.uint8)
    centres = []
    for i, (start, length, sign, d) in enumerate(params):
        cx, cy = origin + pitch * (i % per_row), origin + pitch * (i // per_row)
        put_stamp(img, cx, cy, STAMP_C, start, length, STAMP_C + sign * d)
        centres.append((cx, cy))
    return img, np.array(centres, dtype=np.int32)


def level0_params(b=FIXED_T[0]):
    return [(s, n, sign, d) for d in (b, b + 1) for sign in (1, -1) for n in (9, 10, 11, 16) for s in range(16)]


def level0_expect(params, b=FIXED_T[0]):
    return np.array([n >= 10 and d == b + 1 for (_s, n, _sign, d) in params])


def level0_frames():
    """The 256-stamp sheet at six translations: [(frame 272x272, centres, corner expected at the centre)]."""
    P = level0_params()
    return [stamp_sheet(P, 272, o, 16, 16) + (level0_expect(P),) for o in ORIGINS]


def level_params(l):
    return [(s, n, sign, FIXED_T[l] + 1) for sign in (1, -1) for n in (9, 10) for s in range(16)]


def level_frames(l):
    """The 64-stamp sheet of level l = 1 .. 3, upsampled by 2^l: [(frame, sheet, centres at level l, corner expected)].  Levels 1 and 2:
    six translations at pitch 16.  Level 3: one 1024x1024 frame at pitch 15, whose eight centres per axis take every residue modulo 8."""
    P = level_params(l)
    exp = np.array([n >= 10 for (_s, n, _sign, _d) in P])
    out = []
    for sheet, centres in ([stamp_sheet(P, 160, o, 16, 8) for o in ORIGINS] if l < 3 else [stamp_sheet(P, 128, 8, 15, 8)]):
        out.append((np.kron(sheet, np.ones((1 << l, 1 << l), dtype=np.uint8)), sheet, centres, exp))
    return out


SCORE_STAMPS = ((120, 126), (120, 131), (120, 151), (120, 220), (0, 255), (255, 0))      # (centre, ring), full ring
SCORE_EXPECT = (5, 10, 30, 99, 254, 254)


def score_frame():
    """Six arc-16 stamps, each on a flat cell of its centre value, 32 pixels from the top: (frame 128x64, centres, expected scores)."""
    img = np.zeros((64, 128), dtype=np.uint8)
    centres = []
    for i, (c, r) in enumerate(SCORE_STAMPS):
        cx = 16 + 16 * i
        img[:, cx - 8:cx + 8] = c
        if i == 0:
            img[:, :cx - 8] = c
        if i == len(SCORE_STAMPS) - 1:
            img[:, cx + 8:] = c
        put_stamp(img, cx, 32, c, 0, 16, r)
        centres.append((cx, 32))
    return img, np.array(centres, dtype=np.int32), np.array(SCORE_EXPECT)


# ------------------------------------------------------------------------------------------------ 2. tile-size seams
SEAM_SIZES = ((64, 64), (65, 64), (64, 65), (71, 73), (127, 129), (128, 128), (135, 137), (193, 67), (240, 208))


def seam_images(w, h):
    return {"noise": noise(w, h, 1000 * w + h), "octaves": multi_octave(w, h, 1000 * w + h + 1, amp=90 + (7 * w + 3 * h) % 31)}


def strided(img, pad):
    """The same pixels as a row-strided view (row stride w + pad) of a larger array filled with 255."""
    h, w = img.shape
    big = np.full((h, w + pad), 255, dtype=np.uint8)
    big[:, :w] = img
    return big[:, :w]


# ------------------------------------------------------------------------------------------------ 3. row tables
ROW_SHAPES = tuple((64, h) for h in (64, 65, 66, 67, 257, 260, 513, 516)) + tuple((w, h) for w in (65, 127, 129, 193) for h in (64, 65, 66, 67))
SPARSE_SHAPE = (193, 67)
SPARSE_NAMES = ("first_row", "last_row", "one", "none", "even_rows", "x_ge_64", "x_lt_64")
BATCH_SHAPES = ((64, 516), (128, 64), (65, 67))


def sparse_subsets(corners, w, h):
    c = np.asarray(corners)
    x, y = c[:, 0], c[:, 1]
    sel = {"first_row": y == 3, "last_row": y == h - 4, "one": np.arange(len(c)) == len(c) // 2, "none": np.zeros(len(c), dtype=bool),
           "even_rows": y % 2 == 0, "x_ge_64": x >= 64, "x_lt_64": x < 64}
    return {k: c[v] for k, v in sel.items()}


def row_cases():
    """[(name, w, h, image, masks or None)] of section 3: noise at every shape, and the sparse frames made from the unmasked oracle run."""
    from oracle import OracleKeyFrame
    out = [("noise_%dx%d" % (w, h), w, h, noise(w, h, 31 * w + h), None) for (w, h) in ROW_SHAPES]
    w, h = SPARSE_SHAPE
    img = noise(w, h, 31 * w + h)
    o = OracleKeyFrame(w, h)
    o.MakeKeyFrame_Lite(img)
    for name, sub in sparse_subsets(o.Corners(0), w, h).items():
        out.append(("sparse_" + name, w, h, img, subset_masks(w, h, sub)))
    return out


def tables_of(kf):
    """What MakeKeyFrame_Lite leaves in a KeyFrame or an OracleKeyFrame besides the images: {key: array}."""
    out = {}
    for l in range(LEVELS):
        out["corners%d" % l] = np.asarray(kf.Corners(l), dtype=np.int32).reshape(-1, 2)
        out["lut%d" % l] = np.asarray(kf.RowLUT(l), dtype=np.int32)
        out["thresh%d" % l] = np.array(kf.FastThresh(l))
        out["hist%d" % l] = np.asarray(kf.FastFrequency(l), dtype=np.float64)
    return out


def run_row_cases(make_kf, batch=None):
    """Every row_cases() frame on a fresh handle of make_kf(w, h), then the three cameras of BATCH_SHAPES run twice (through
    batch(kfs, frames) if given, else one by one), then the reuse sequence noise, black, noise on one handle.  {"<case>/<key>": array}."""
    out = {}

    def keep(name, kf):
        for k, v in tables_of(kf).items():
            out[name + "/" + k] = v
    for name, w, h, img, masks in row_cases():
        kf = make_kf(w, h)
        kf.MakeKeyFrame_Lite(img, masks)
        keep(name, kf)
    kfs = [make_kf(w, h) for (w, h) in BATCH_SHAPES]
    for rep in range(2):
        frames = batch_frames(rep)
        if batch is not None:
            batch(kfs, frames)
        else:
            for kf, f in zip(kfs, frames):
                kf.MakeKeyFrame_Lite(f)
        for c, kf in enumerate(kfs):
            keep("batch%d_cam%d" % (rep, c), kf)
    w, h = 129, 67
    kf = make_kf(w, h)
    for i, f in enumerate(reuse_frames(w, h)):
        kf.MakeKeyFrame_Lite(f)
        keep("reuse%d" % i, kf)
    return out


def batch_frames(rep):
    return [noise(w, h, 77 * w + h + rep) for (w, h) in BATCH_SHAPES]


def reuse_frames(w, h):
    a = noise(w, h, 5)
    return [a, np.zeros((h, w), dtype=np.uint8), a]


# ------------------------------------------------------------------------------------------------ 4. candidates
CAND_SIZE = (128, 128)
CAND_COUNTS = (1, 255, 256, 257, 512, 513)
REST_PARAMS = ((False, True, 0), (True, True, 0), (True, False, 0), (False, True, 1))      # (use_shi, use_percent, nonmax_score)


def cand_image():
    return noise(CAND_SIZE[0], CAND_SIZE[1], 4242)


def in_border(c, w, h, b=10):
    c = np.asarray(c).reshape(-1, 2)
    return (c[:, 0] >= b) & (c[:, 1] >= b) & (c[:, 0] < w - b) & (c[:, 1] < h - b)


def candidate_subsets(corners, scores, w, h):
    """Index sets into the unmasked corner list (ascending = raster order), by name; scores are the FAST scores of the corners.
    A name whose subset cannot be built from this list is left out (the CPU test asserts that none is)."""
    rng = np.random.default_rng(99)
    C = np.asarray(corners)
    n = len(C)
    where = {(int(x), int(y)): i for i, (x, y) in enumerate(C)}
    inb = in_border(C, w, h)
    out = {}
    for N in CAND_COUNTS:
        out["count_%d" % N] = np.sort(rng.choice(n, N, replace=False))
    # a pair adjacent in x (dx = 1) or y (dy = 1), first at index 255, second at 256, both inside the border, by the order of their scores
    for axis, (dx, dy) in (("x", (1, 0)), ("y", (0, 1))):
        for rel, test in (("gt", lambda a, b: a > b), ("lt", lambda a, b: a < b), ("eq", lambda a, b: a == b)):
            for i in range(n - 1, 254, -1):
                j = where.get((int(C[i, 0]) + dx, int(C[i, 1]) + dy))
                if j is None or not (inb[i] and inb[j]) or not test(scores[i], scores[j]):
                    continue
                # the pair stands alone: no other corner of the subset touches either of the two
                alone = (np.abs(C - C[i]).max(axis=1) > 1) & (np.abs(C - C[j]).max(axis=1) > 1)
                before = np.sort(rng.choice(np.nonzero(alone[:i])[0], 255, replace=False))
                after = (j + 1 + np.nonzero(alone[j + 1:])[0])[:40]
                out["pair_%s_%s" % (axis, rel)] = np.concatenate([before, [i, j], after])
                break
    # only corner index 256 / 512 lies inside the border: every corner before it fails the border test
    outside = np.nonzero(~inb)[0]
    for N in (256, 512):
        ks = [k for k in range(n) if 12 <= C[k, 0] < w - 12 and 12 <= C[k, 1] < h - 12 and np.searchsorted(outside, k) >= N]
        if ks:
            k = ks[0]
            out["border_only_%d" % N] = np.concatenate([outside[outside < k][-N:], [k]])
    lines = np.isin(C[:, 0], (9, 10, w - 11, w - 10)) | np.isin(C[:, 1], (9, 10, h - 11, h - 10))
    out["border_lines"] = np.union1d(np.nonzero(lines)[0], rng.choice(n, 100, replace=False))
    out["second_frame"] = np.sort(rng.choice(n, 300, replace=False))
    return out


CAND_TALL_SIZE = (128, 256)
CAND_NAMES = tuple("count_%d" % n for n in CAND_COUNTS) + tuple("pair_%s_%s" % (a, r) for a in "xy" for r in ("gt", "lt", "eq")) + \
    ("border_only_256", "border_only_512", "border_lines", "second_frame")


def candidate_cases():
    """{name: (frame, corners of the subset, their FAST scores)} for every name of CAND_NAMES that can be built.  All on the 128x128
    noise frame but border_only_512: the 128x128 frame has fewer than 512 corners outside the border (about 470), so that one case
    uses a 128x256 noise frame (about 640 of them before its last interior corner)."""
    from oracle import OracleKeyFrame
    out = {}
    for (w, h), img, names in ((CAND_SIZE, cand_image(), None), (CAND_TALL_SIZE, noise(CAND_TALL_SIZE[0], CAND_TALL_SIZE[1], 4243), ("border_only_512",))):
        o = OracleKeyFrame(w, h)
        o.MakeKeyFrame_Lite(img)
        C = o.Corners(0)
        S = fast_scores(img, C)
        for name, idx in candidate_subsets(C, S, w, h).items():
            if name not in out and (names is None or name in names):
                out[name] = (img, C[idx], S[idx])
    return out


# ------------------------------------------------------------------------------------------------ 5. MiniPatch
MP_SIZE = (128, 128)
MP_RANGE = 10
MP_BIG_RANGES = (11, 16, 200)              # windows of 23^2 and 33^2 pixels at about 0.13 corners per pixel, and the whole frame


def minipatch_images():
    """(source, destination): noise, and the same noise moved by at most 2 grey levels, so true matches have a small non-zero SSD."""
    w, h = MP_SIZE
    a = noise(w, h, 808, hi=250).astype(np.int32) + 3
    d = np.random.default_rng(809).integers(-2, 3, size=(h, w))
    return a.astype(np.uint8), (a + d).astype(np.uint8)


def _snap(corners, x, y, w, h):
    """the corner with a whole 9x9 patch that lies nearest to (x, y)"""
    c = np.asarray(corners)
    ok = (c[:, 0] >= 4) & (c[:, 1] >= 4) & (c[:, 0] < w - 4) & (c[:, 1] < h - 4)
    c = c[ok]
    return c[np.argmin((c[:, 0] - x) ** 2 + (c[:, 1] - y) ** 2)]


def minipatch_positions(dst_corners):
    """{range: (src_pos, dst_pos)} of the clamp and window cases; dst_corners = level-0 corners of the destination frame."""
    w, h = MP_SIZE
    r = MP_RANGE
    src, dst = [], []
    for v in (3, 4, w - 5, w - 4):                      # source patch on either side of the 4-pixel border
        for sp in ((v, 60), (60, v)):
            src.append(sp)
            dst.append(tuple(_snap(dst_corners, sp[0], sp[1], w, h)))
    ys = [t + r for t in (-5, 0, h - 1, h + 3)] + [b - r for b in (-3, -2, -1, h - 2, h - 1, h + 5)]
    for y in ys:
        for x in (40, 90):
            dst.append((x, y))
            src.append(tuple(_snap(dst_corners, x, y, w, h)))
    for x in (2, w - 2, -r, w - 1 + r):                 # windows that hang over the side edges
        dst.append((x, 64))
        src.append(tuple(_snap(dst_corners, x, 64, w, h)))
    out = {r: (np.array(src, dtype=np.int32), np.array(dst, dtype=np.int32))}
    for big in MP_BIG_RANGES:                           # > 64, > 128, all corners in the window
        d = [(64, 64), (30, 100), (100, 20)]
        out[big] = (np.array([_snap(dst_corners, x, y, w, h) for x, y in d], dtype=np.int32), np.array(d, dtype=np.int32))
    return out


def corners_in_window(corners, pos, rng):
    c = np.asarray(corners)
    return int(((np.abs(c[:, 0] - pos[0]) <= rng) & (np.abs(c[:, 1] - pos[1]) <= rng)).sum())


def periodic_image():
    return np.tile(noise(16, 16, 1616), (MP_SIZE[1] // 16, MP_SIZE[0] // 16))


def tie_case(corners):
    """From the unmasked corners of periodic_image(): a corner subset (as an index array) in which A and B = A + (0, 16) are exactly 64
    indices apart and C and D = C + (16, 0) fewer than 64, and the searches whose windows hold exactly those tied pairs.
    Returns (subset indices, dict(A, B, C, D), src_pos, dst_pos, range, expected winners)."""
    Cn = np.asarray(corners)
    where = {(int(x), int(y)): i for i, (x, y) in enumerate(Cn)}
    iA = next(i for i, (x, y) in enumerate(Cn) if 24 <= x < 104 and 36 <= y < 44 and (int(x), int(y) + 16) in where)
    A = Cn[iA]
    iB = where[(int(A[0]), int(A[1]) + 16)]
    between = [i for i in range(iA + 1, iB) if not ((Cn[i, 0] - A[0]) % 16 == 0 and (Cn[i, 1] - A[1]) % 16 == 0)]
    fill = np.random.default_rng(7).choice(between, 63, replace=False)
    iC = next(i for i, (x, y) in enumerate(Cn) if 24 <= x < 88 and y >= A[1] + 30 and y < 110 and (int(x) + 16, int(y)) in where)
    Cc = Cn[iC]
    iD = where[(int(Cc[0]) + 16, int(Cc[1]))]
    idx = np.sort(np.concatenate([np.arange(0, iA, 7), [iA], fill, [iB], np.arange(iC, iD + 1)]))
    B, D = Cn[iB], Cn[iD]
    src = np.array([A, B, Cc, D], dtype=np.int32)
    dst = np.array([(A[0], A[1] + 8), (A[0], A[1] + 8), (Cc[0] + 8, Cc[1]), (Cc[0] + 8, Cc[1])], dtype=np.int32)
    win = np.array([A, A, Cc, Cc], dtype=np.int32)
    return idx, dict(A=A, B=B, C=Cc, D=D), src, dst, 8, win


# ------------------------------------------------------------------------------------------------ 6. glare
GLARE_SIZES = ((64, 64), (71, 73))


def glare_frames(w, h):
    """Noise of at most 245 with designed saturated pixels: {name: frame}."""
    base = noise(w, h, 600 + w, hi=246)
    out = {}
    f = base.copy()
    for (x, y) in ((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (w // 2, h // 2)):
        f[y, x] = 246
    out["corners_and_centre"] = f
    f = base.copy()
    for (x, y) in ((w // 2, 0), (w // 2, h - 1), (0, h // 2), (w - 1, h // 2)):
        f[y, x] = 255
    out["mid_edges"] = f
    f = np.minimum(base, 244)
    f[h // 3, w // 3] = 245                             # not glare
    f[2 * h // 3, 2 * w // 3] = 246                     # glare
    out["245_and_246"] = f
    f = base.copy()
    f[0, :] = 255
    f[:, w - 1] = 255
    out["row0_and_last_column"] = f
    return out


def glare_caller_masks(w, h):
    out = []
    for l in range(LEVELS):
        m = np.full((h >> l, w >> l), 255, dtype=np.uint8)
        m[:, :(w >> l) // 3] = 0
        m[(h >> l) // 2, :] = 254
        out.append(m)
    return out


if __name__ == "__main__":
    # the child of the route-0 test: the section-3 cases on the device, tables saved to argv[1]
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from mcptam_amd.keyframe import KeyFrame, make_lite_batch
    np.savez(sys.argv[1], knob=np.array(os.environ.get("MCP_IMG_ROW_TABLES", "")), **run_row_cases(KeyFrame, make_lite_batch))

"""Inputs for the edge tests of the feature-initialisation image operators (Shi-Tomasi detector, multi-ellipse patch
search), shared by the CPU anchors (test_oracle_feature_init.py) and the GPU tests (test_gpu_feature_init_edges.py).

Every case names the edge it is built to reach and carries a check() that proves, from the two NumPy restatements below
(eigen_map, ellipse_boxes) and the oracle's answer alone, that it reaches it: a test that compares the device with the
oracle therefore cannot silently miss its edge.  Nothing here touches the device."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

# The thresholds at which the device code takes another path.  They mirror constants of
# scenelib2_amd/csrc/sl2_improc_dev.hpp; if one of those moves, move it here as well.
ME_CAP = 2048            # kMeCap: positions of a union's bounding box the one-workgroup search keeps in LDS
ME_IMG_CAP = 6144        # kMeImgCap: bytes of image under that box (+ 5 pixels all round) kept in LDS
ME_ELL_CAP = 256         # kMeEllCap: ellipses of a job the one-workgroup search takes
ME_HALF_COLS = 32        # two ellipses share a wavefront, a half each, when both boxes are at most this wide
ME_WAVE_COLS = 64        # me_for_each_inside: a lane keeps one column per block of 64
ME_BAND_BYTES = 16384    # kMeBandBytes: the many-workgroup form's LDS band of image rows
ME_BIG_SLICES = 64       # kMeBigSlices: row slices of a union in k_me_big_scores
ME_BIG_PARTS = 16        # kMeBigArgWaves: row parts of an ellipse's box in k_me_big_argmin
ME_BIG_GRID_X = 128      # kMeBigGridX: ellipses of a job in flight in k_me_big_argmin
ME_BIG_GRID_Y = 8        # kMeBigGridY: jobs in flight in both k_me_big_* kernels
DET_TW, DET_TH = 80, 60  # kDetTW x kDetTH: the detector's tile of positions
DET_SEG = 8              # columns of a tile row one thread sums by sliding
DET_THREADS = 1024       # kDetThreads: position i of a tile belongs to thread i % 1024
BOX = 11                 # kBoxSize
HALF = 5


# ---------------------------------------------------------------------------------------------------------------------
# images
# ---------------------------------------------------------------------------------------------------------------------
def texture(rng, H, W):
    """Smoothed noise: no two positions score equally."""
    img = rng.integers(0, 256, (H, W)).astype(np.float64)
    k = np.array([1, 4, 6, 4, 1.0]); k /= k.sum()
    for ax in (0, 1):
        img = np.apply_along_axis(lambda m: np.convolve(m, k, mode="same"), ax, img)
    img = (img - img.min()) / (img.max() - img.min()) * 255
    return img.astype(np.uint8)


def periodic(rng, H, W, ph, pw):
    """A random ph x pw tile repeated: every window has exact copies (ph, pw) apart, so every score is attained often."""
    tile = rng.integers(0, 256, (ph, pw)).astype(np.uint8)
    return np.tile(tile, (H // ph + 1, W // pw + 1))[:H, :W].copy()


# ---------------------------------------------------------------------------------------------------------------------
# detector: NumPy restatement
# ---------------------------------------------------------------------------------------------------------------------
def gradient_sums(img):
    """The three 11 x 11 box sums of products of the doubled central differences, int64, at every position; meaningful where
    6 <= u < W - 6 and 6 <= v < H - 6 (elsewhere the window leaves the gradients' support)."""
    I = img.astype(np.int64)
    H, W = I.shape
    gx = np.zeros_like(I); gy = np.zeros_like(I)
    gx[:, 1:-1] = I[:, 2:] - I[:, :-2]
    gy[1:-1, :] = I[2:, :] - I[:-2, :]
    out = []
    for prod in (gx * gx, gx * gy, gy * gy):
        c = np.zeros((H + 1, W + 1), np.int64)
        c[1:, 1:] = prod.cumsum(0).cumsum(1)
        s = np.zeros_like(I)
        s[HALF:H - HALF, HALF:W - HALF] = c[BOX:, BOX:] - c[:-BOX, BOX:] - c[BOX:, :-BOX] + c[:-BOX, :-BOX]
        out.append(s)
    return out


def eigen_map(img):
    """The detector's smaller eigenvalue at every valid position (-inf elsewhere): integer sums, then the reference's FP64
    expression (monoslam.cpp:1194-1205) in its order."""
    sxx, sxy, syy = gradient_sums(img)
    A = sxx / 4.0; B = sxy / 4.0; C = syy / 4.0
    with np.errstate(invalid="ignore"):
        e2 = (A + C - np.sqrt((A + C) * (A + C) - 4 * (A * C - B * B))) / 2.0
    H, W = img.shape
    out = np.full((H, W), -np.inf)
    out[6:H - 6, 6:W - 6] = e2[6:H - 6, 6:W - 6]
    return out


def clamp_region(region, W, H):
    us, vs, uf, vf = (int(x) for x in region)
    return max(us, 6), max(vs, 6), min(uf, W - 6), min(vf, H - 6)


def detector_expected(emap, region, uv_in):
    """(u, v, evbest) by the reference's rule - v outer, u inner, strict '>' from 0: the FIRST maximum - and the list of all
    positions (u, v) that attain the maximum."""
    H, W = emap.shape
    us, vs, uf, vf = clamp_region(region, W, H)
    if vs >= vf or us >= uf:
        return (us, vs, 0.0), []
    sub = emap[vs:vf, us:uf]
    sub = np.where(np.isnan(sub), -np.inf, sub)            # a NaN never compares greater
    best = sub.max()
    if not best > 0.0:
        return (int(uv_in[0]), int(uv_in[1]), 0.0), []
    rv, cu = np.nonzero(sub == best)                        # row-major = v outer, u inner
    return (us + int(cu[0]), vs + int(rv[0]), float(best)), [(us + int(c), vs + int(r)) for r, c in zip(rv, cu)]


def detector_tiles(positions, region, W, H):
    """The detector's tiles (counted from the clamped region's origin) that hold the given positions."""
    us, vs, _, _ = clamp_region(region, W, H)
    return {((u - us) // DET_TW, (v - vs) // DET_TH) for u, v in positions}


# ---------------------------------------------------------------------------------------------------------------------
# multi-ellipse search: NumPy restatement of the boxes
# ---------------------------------------------------------------------------------------------------------------------
def ellipse_boxes(puinv, centre, W, H):
    """Per ellipse (uc, vc, us, nu, vs, nv): the truncated centre and the clipped box of relative offsets us .. us + nu - 1,
    vs .. vs + nv - 1 (search_multiple_overlapping_ellipses.cpp:43-51, 127-149); nu or nv <= 0: no position.  And the
    bounding box (x0, y0, bw, bh) of the union of the valid boxes, None without one."""
    boxes = []
    lo_x = lo_y = None
    hi_x = hi_y = None
    for (a, b, c), (cu, cv) in zip(np.asarray(puinv, dtype=np.float64).reshape(-1, 3), np.asarray(centre, dtype=np.float64).reshape(-1, 2)):
        hw = int(3.0 / np.sqrt(a - b * b / c))
        hh = int(3.0 / np.sqrt(c - b * b / a))
        uc, vc = int(cu), int(cv)                           # truncation towards zero, no + 0.5
        us, uf, vs, vf = -hw, hw, -hh, hh
        if uc + us - HALF < 0: us = HALF - uc
        if uc + uf - HALF > W - BOX: uf = W - BOX - uc + HALF
        if vc + vs - HALF < 0: vs = HALF - vc
        if vc + vf - HALF > H - BOX: vf = H - BOX - vc + HALF
        nu, nv = uf - us + 1, vf - vs + 1
        boxes.append((uc, vc, us, nu, vs, nv))
        if nu > 0 and nv > 0:
            x, y = uc + us, vc + vs
            lo_x = x if lo_x is None else min(lo_x, x); lo_y = y if lo_y is None else min(lo_y, y)
            hi_x = x + nu if hi_x is None else max(hi_x, x + nu); hi_y = y + nv if hi_y is None else max(hi_y, y + nv)
    union = None if lo_x is None else (lo_x, lo_y, hi_x - lo_x, hi_y - lo_y)
    return boxes, union


def inside(pu, urel, vrel):
    a, b, c = (float(x) for x in pu)
    return a * urel * urel + 2 * b * urel * vrel + c * vrel * vrel < 9.0


def me_form(boxes, union):
    """Which form of the search a job takes: 'none' (no valid box), 'lds' (one workgroup, image tile in LDS), 'memory' (one
    workgroup, scored from memory), 'big' (many workgroups)."""
    if len(boxes) > ME_ELL_CAP:
        return "big"
    if union is None:
        return "none"
    _, _, bw, bh = union
    if bw * bh > ME_CAP:
        return "big"
    return "lds" if (bw + 10) * (bh + 10) <= ME_IMG_CAP else "memory"


def tied_positions(img, pu, box, best_uv):
    """Box-relative (q, r) of the ellipse's positions whose 11 x 11 window equals, byte for byte, the window at best_uv: they
    score exactly what best_uv scores.  In scan order (u outer, v inner)."""
    uc, vc, us, nu, vs, nv = box
    win = sliding_window_view(img, (BOX, BOX))               # [y - 5][x - 5]
    x0, y0 = uc + us, vc + vs
    same = (win[y0 - HALF:y0 - HALF + nv, x0 - HALF:x0 - HALF + nu] == win[best_uv[1] - HALF, best_uv[0] - HALF]).all(axis=(2, 3))
    return [(q, r) for q in range(nu) for r in range(nv) if same[r, q] and inside(pu, us + q, vs + r)]


def me_lane(q, r, nu, lanes, r_first=0):
    """The lane of me_for_each_inside that meets position (q, r) of a box nu wide (lanes = 32: half a wavefront)."""
    lg = 4 if nu <= 16 else (5 if nu <= ME_HALF_COLS else 6)
    rp = lanes >> lg
    return (q % ME_WAVE_COLS) % (1 << lg) + (((r - r_first) % rp) << lg)


def me_half_mode(boxes, e):
    """Whether ellipse e of a one-workgroup job is walked by half a wavefront (it and its partner at most 32 columns)."""
    e0 = e & ~1
    pair = [boxes[e0][3]] + ([boxes[e0 + 1][3]] if e0 + 1 < len(boxes) else [])
    return all(nu <= ME_HALF_COLS for nu in pair)


TIE_KINDS = ("same_lane", "cross_lane", "cross_half", "cross_block", "cross_part")


def tie_kinds(boxes, e, ties, form):
    """Which reductions of the arg-min the tied positions of ellipse e straddle."""
    nu, nv = boxes[e][3], boxes[e][5]
    kinds = set()
    rows_per = (nv + ME_BIG_PARTS - 1) // ME_BIG_PARTS
    lanes = 64 if form == "big" or not me_half_mode(boxes, e) else 32
    for i, (q1, r1) in enumerate(ties):
        for q2, r2 in ties[i + 1:]:
            if q1 // ME_WAVE_COLS != q2 // ME_WAVE_COLS:
                kinds.add("cross_block")
            if form == "big" and r1 // rows_per != r2 // rows_per:
                kinds.add("cross_part")                     # met by different wavefronts: no lane relation
                continue
            first = (r1 // rows_per) * rows_per if form == "big" else 0
            l1, l2 = me_lane(q1, r1, nu, lanes, first), me_lane(q2, r2, nu, lanes, first)
            if l1 == l2:
                kinds.add("same_lane")
            else:
                kinds.add("cross_lane")
                if lanes == 64 and l1 // 32 != l2 // 32:
                    kinds.add("cross_half")
    return kinds


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
class DetCase:
    """One call of find_best_patch_batch.  check(want) with want[t] = the oracle's (u, v, evbest) of job t."""

    def __init__(self, name, edge, images, idx, regions, check, uv_in=(-3, -4)):
        self.name, self.edge = name, edge
        self.images = np.ascontiguousarray(images, dtype=np.uint8)
        self.idx = np.array(idx, np.int32)
        self.regions = np.array(regions, np.int32).reshape(-1, 4)
        self.uv_in = np.tile(np.array([uv_in], np.int32), (len(self.regions), 1))
        self._check = check
        self._emaps = {}
        self._want = None

    def __repr__(self):
        return "DetCase(%s)" % self.name

    @property
    def W(self):
        return self.images.shape[2]

    @property
    def H(self):
        return self.images.shape[1]

    def emap(self, i):
        if i not in self._emaps:
            self._emaps[i] = eigen_map(self.images[i])
        return self._emaps[i]

    def numpy_expected(self, t):
        return detector_expected(self.emap(int(self.idx[t])), self.regions[t], self.uv_in[t])

    def clamped_size(self, t):
        us, vs, uf, vf = clamp_region(self.regions[t], self.W, self.H)
        return uf - us, vf - vs

    def oracle(self, oa):
        if self._want is None:
            self._want = [oa.find_best_patch(self.images[self.idx[t]], self.regions[t], self.uv_in[t]) for t in range(len(self.regions))]
        return self._want

    def check(self, want):
        """The oracle equals the NumPy restatement on every job, and the case reaches its edge."""
        for t in range(len(self.regions)):
            assert tuple(want[t]) == self.numpy_expected(t)[0], (self.name, t, list(self.regions[t]), want[t], self.numpy_expected(t)[0])
        self._check(self, want)


class MeCase:
    """One call of search_multiple_overlapping_ellipses_batch; jobs = [(image index, patch, [(a, b, c, cu, cv), ...])].
    check(want) with want[j] = the oracle's (result [n][3], corrmax [n], positions correlated) of job j."""

    def __init__(self, name, edge, images, jobs, check):
        self.name, self.edge = name, edge
        self.images = np.ascontiguousarray(images, dtype=np.uint8)
        self.idx = np.array([j[0] for j in jobs], np.int32)
        self.patches = np.stack([np.asarray(j[1], np.uint8).reshape(121) for j in jobs])
        self.counts = np.array([len(j[2]) for j in jobs], np.int32)
        ell = np.array([e for j in jobs for e in j[2]], dtype=np.float64).reshape(-1, 5)
        self.pu, self.ce = np.ascontiguousarray(ell[:, :3]), np.ascontiguousarray(ell[:, 3:])
        self.first = np.concatenate([[0], np.cumsum(self.counts)])
        self._check = check
        self._want = None

    def __repr__(self):
        return "MeCase(%s)" % self.name

    @property
    def W(self):
        return self.images.shape[2]

    @property
    def H(self):
        return self.images.shape[1]

    def sl(self, j):
        return slice(int(self.first[j]), int(self.first[j + 1]))

    def boxes(self, j):
        return ellipse_boxes(self.pu[self.sl(j)], self.ce[self.sl(j)], self.W, self.H)

    def form(self, j):
        return me_form(*self.boxes(j))

    def ties(self, j, e, want):
        """Tied minimal positions of ellipse e of job j: the positions that look exactly like the oracle's answer."""
        boxes, _ = self.boxes(j)
        res = want[j][0]
        return tied_positions(self.images[self.idx[j]], self.pu[self.sl(j)][e], boxes[e], (int(res[e, 1]), int(res[e, 2])))

    def tie_kinds(self, j, e, want):
        boxes, union = self.boxes(j)
        return tie_kinds(boxes, e, self.ties(j, e, want), "big" if me_form(boxes, union) == "big" else "one")

    def oracle(self, oa):
        if self._want is None:
            self._want = [oa.search_multiple_ellipses(self.images[self.idx[j]], self.patches[j], self.pu[self.sl(j)], self.ce[self.sl(j)])
                          for j in range(len(self.counts))]
        return self._want

    def check(self, want):
        self._check(self, want)


def _cut(img, cx, cy):
    return img[cy - HALF:cy + HALF + 1, cx - HALF:cx + HALF + 1].copy()


def _diag(hw, hh):
    """S^-1 of an axis-aligned ellipse whose half-width / half-height truncate to hw / hh."""
    return 9.0 / (hw + 0.5) ** 2, 0.0, 9.0 / (hh + 0.5) ** 2


def _sinv(s00, s01, s11):
    det = s00 * s11 - s01 * s01
    return s11 / det, -s01 / det, s00 / det


# ----- detector ------------------------------------------------------------------------------------------------------
DW, DH = 203, 151        # odd width; 191 x 139 valid positions = 3 x 3 tiles
DET_TEX, DET_PERIODIC, DET_VSTRIPES, DET_HSTRIPES, DET_DIAG, DET_CHECKER1, DET_CHECKER2, DET_BLOBS, DET_BLOBS_NEAR, DET_LAST = range(10)


def _detector_pool():
    rng = np.random.default_rng(1234)
    u, v = np.meshgrid(np.arange(DW), np.arange(DH))
    blobs = np.full((DH, DW), 100, np.uint8)
    blob = rng.integers(0, 256, (9, 9)).astype(np.uint8)
    blobs[30:39, 120:129] = blob                            # first in scan order (row 30), in the SECOND tile column
    blobs[44:53, 20:29] = blob                              # met first when tiles are walked one after the other
    # the same, 16 columns left and 12 rows down of one tile further: (12 * 80 + 64) % 1024 == 0, ONE thread meets both
    near = np.full((DH, DW), 100, np.uint8)
    near[20:29, 88:97] = blob
    near[32:41, 72:81] = blob
    return np.stack([
        texture(rng, DH, DW),
        periodic(rng, DH, DW, 9, 7),
        (40 + 170 * ((u // 3) % 2)).astype(np.uint8),       # vertical stripes: gy = 0
        (40 + 170 * ((v // 3) % 2)).astype(np.uint8),       # horizontal stripes: gx = 0
        (40 + 170 * (((u + v) // 3) % 2)).astype(np.uint8),  # 45 degrees: gx = gy
        (255 * ((u + v) % 2)).astype(np.uint8),             # one-pixel checkerboard: both central differences vanish
        (255 * (((u // 2) + (v // 2)) % 2)).astype(np.uint8),  # two-pixel checkerboard: |2 gx| = |2 gy| = 255 everywhere
        blobs,
        near,
        texture(rng, DH, DW),
    ])


DET_SIZES = ([(1, 1), (1, 23), (37, 1), (1, 61), (81, 1)] + [(w, 5) for w in range(2, 18)] + [(w, 11) for w in range(73, 88)] +
             [(79, 59), (80, 60), (81, 61), (79, 61), (81, 59), (80, 59), (80, 61), (93, 67), (159, 119), (160, 120), (161, 121),
              (161, 60), (80, 121)])
DET_SIZES_REQUIRED = ([(1, 1), (160, 120), (161, 121)], [1, 7, 8, 9, 15, 16, 17, 79, 80, 81], [1, 59, 60, 61])


def _det_size_jobs():
    idx, regions, sizes = [], [], []
    for k, (nu, nv) in enumerate(DET_SIZES):
        for us, vs in ((6, 6), (11, 8), (DW - 6 - nu, DH - 6 - nv)):
            regions.append([us, vs, us + nu, vs + nv]); idx.append(DET_LAST if k % 2 else DET_TEX); sizes.append((nu, nv))
    return idx, regions, sizes


def _check_det_sizes(case, want):
    _, _, sizes = _det_size_jobs()
    got = [case.clamped_size(t) for t in range(len(case.regions))]
    assert got == sizes
    exact, widths, heights = DET_SIZES_REQUIRED
    assert set(exact) <= set(got) and set(widths) <= {s[0] for s in got} and set(heights) <= {s[1] for s in got}
    rem_first = {nu % DET_SEG for nu, _ in got if nu < DET_TW}                       # the remainder in the first (only) tile
    rem_own = {nu - DET_TW for nu, _ in got if DET_TW < nu < DET_TW + DET_SEG}       # ... alone in a tile of its own
    rem_last = {(nu % DET_TW) % DET_SEG for nu, _ in got if nu % DET_TW > DET_SEG}   # ... after whole segments of the last tile
    assert rem_first >= set(range(1, 8)) and rem_own >= set(range(1, 8)) and rem_last - {0}
    assert all(w[2] > 0.0 for w in want)                    # a texture: every region has a winner


DET_CLAMP = [  # region, the coordinates the clamp must move (0 us, 1 vs, 2 uf, 3 vf), image
    ([-10, 40, 30, 80], {0}, DET_TEX), ([DW - 30, 40, DW + 9, 80], {2}, DET_TEX), ([50, -7, 90, 30], {1}, DET_TEX),
    ([50, DH - 25, 90, DH + 3], {3}, DET_TEX), ([-4, -4, 40, 30], {0, 1}, DET_TEX), ([DW - 40, -1, DW, 30], {1, 2}, DET_TEX),
    ([0, DH - 30, 40, DH], {0, 3}, DET_TEX), ([DW - 40, DH - 30, DW + 1, DH + 1], {2, 3}, DET_TEX),
    ([-5, -5, DW + 5, DH + 5], {0, 1, 2, 3}, DET_TEX), ([DW - 20, DH - 20, DW + 5, DH + 5], {2, 3}, DET_LAST),
    ([DW - 7, DH - 7, DW, DH], {2, 3}, DET_LAST),            # one position: the bottom-right corner of the last image
    ([DW - 6, 40, DW + 9, 80], {2}, DET_LAST), ([30, DH - 6, 60, DH], {3}, DET_LAST),   # clamped to nothing
]


def _check_det_clamp(case, want):
    for t, (reg, moved, _) in enumerate(DET_CLAMP):
        cl = clamp_region(reg, DW, DH)
        assert {k for k in range(4) if cl[k] != reg[k]} == moved, (t, reg, cl)
    sizes = [case.clamped_size(t) for t in range(len(DET_CLAMP))]
    assert sizes[10] == (1, 1) and want[10][:2] == (DW - 7, DH - 7) and case.idx[10] == len(case.images) - 1
    assert sizes[11][0] == 0 and sizes[12][1] == 0 and want[11] == (DW - 6, 40, 0.0) and want[12] == (30, DH - 6, 0.0)
    assert all(s[0] > 0 and s[1] > 0 for s in sizes[:11])


def _check_det_tiny13(case, want):
    assert case.W == 13 and case.H == 13
    for i in range(len(case.images)):
        assert np.isfinite(case.emap(i)).sum() == 1 and case.emap(i)[6, 6] > 0.0      # the single valid position
    assert [w[:2] for w in want] == [(6, 6), (6, 6), (6, 6), (7, 7), (6, 6), (6, 6), (6, 6)]
    assert [w[2] > 0 for w in want] == [True, True, True, False, False, True, True]


def _check_det_tiny14(case, want):
    assert case.W == 14 and case.H == 13
    assert all(np.isfinite(case.emap(i)).sum() == 2 for i in range(len(case.images)))
    assert {w[:2] for w in want} == {(6, 6), (7, 6)} and all(w[2] > 0.0 for w in want)


DET_TIES = [  # region, image, tiles the maxima must spread over at least
    ([0, 0, DW, DH], DET_PERIODIC, 9), ([20, 15, 120, 85], DET_PERIODIC, 4), ([70, 50, 100, 75], DET_PERIODIC, 1),
    ([6, 6, 86, 66], DET_PERIODIC, 1), ([33, 27, 113, 87], DET_PERIODIC, 1), ([DW - 86, DH - 66, DW - 6, DH - 6], DET_PERIODIC, 1),
    ([6, 6, 87, 67], DET_PERIODIC, 1), ([40, 30, 200, 150], DET_PERIODIC, 4),
    ([0, 0, DW, DH], DET_BLOBS, 2), ([10, 20, 180, 75], DET_BLOBS, 2), ([0, 0, DW, DH], DET_BLOBS_NEAR, 2),
]


def _check_det_ties(case, want):
    for t, (reg, _, ntiles) in enumerate(DET_TIES):
        exp, maxima = case.numpy_expected(t)
        assert len(maxima) >= 2 and maxima[0] == exp[:2] == want[t][:2], (t, len(maxima))
        tiles = detector_tiles(maxima, reg, DW, DH)
        assert len(tiles) >= ntiles, (t, tiles)
    # the two blobs: the first maximum in scan order lies in a later tile than the other one
    for t in (8, 9, 10):
        _, maxima = case.numpy_expected(t)
        first, other = detector_tiles(maxima[:1], DET_TIES[t][0], DW, DH), detector_tiles(maxima[1:], DET_TIES[t][0], DW, DH)
        assert len(maxima) == 2 and min(other) < min(first), (maxima, first, other)
    # ... and in the last of them both belong to the same thread, which meets the later one first
    us, vs, _, _ = clamp_region(DET_TIES[10][0], DW, DH)
    owner = [(((v - vs) % DET_TH) * DET_TW + (u - us) % DET_TW) % DET_THREADS for u, v in case.numpy_expected(10)[1]]
    assert owner[0] == owner[1], owner
    owner = [(((v - vs) % DET_TH) * DET_TW + (u - us) % DET_TW) % DET_THREADS for u, v in case.numpy_expected(8)[1]]
    assert owner[0] != owner[1], owner


DET_FLAT = [DET_VSTRIPES, DET_HSTRIPES, DET_DIAG, DET_CHECKER1]


def _det_structure_jobs():
    idx, regions = [], []
    for i in DET_FLAT + [DET_CHECKER2]:
        for reg in ([0, 0, DW, DH], [30, 20, 110, 80], [100, 70, 117, 75]):
            idx.append(i); regions.append(reg)
    return idx, regions


def _check_det_structure(case, want):
    for t in range(len(case.regions)):
        us, vs, uf, vf = clamp_region(case.regions[t], DW, DH)
        sub = case.emap(int(case.idx[t]))[vs:vf, us:uf]
        if case.idx[t] in DET_FLAT:                         # rank one or flat: the smaller eigenvalue is exactly zero everywhere
            assert (sub == 0.0).all() and want[t] == (-3, -4, 0.0), (t, want[t])
        else:
            assert want[t][2] > 0.0
    valid = (slice(6, DH - 6), slice(6, DW - 6))
    sxx, sxy, syy = (s[valid] for s in gradient_sums(case.images[DET_CHECKER2]))
    assert sxx.max() == syy.max() == 121 * 255 * 255           # the largest sums the detector can meet
    sxx, sxy, syy = (s[valid] for s in gradient_sums(case.images[DET_VSTRIPES]))
    assert sxx.min() > 0 and not syy.any() and not sxy.any()
    sxx, sxy, syy = (s[valid] for s in gradient_sums(case.images[DET_DIAG]))
    assert sxx.min() > 0 and (sxx == sxy).all() and (sxx == syy).all()


def _check_det_many(case, want):
    assert len(case.regions) == 300 and set(case.idx) == set(range(len(case.images)))


def detector_cases():
    pool = _detector_pool()
    rng = np.random.default_rng(77)
    cases = []
    idx, regions, _ = _det_size_jobs()
    cases.append(DetCase("sizes", "clamped nu x nv at 1, the 8-column segment, the 80 x 60 tile and two tiles, +-1", pool, idx, regions,
                         _check_det_sizes))
    cases.append(DetCase("clamp", "regions over each border and corner, the last image's corner, clamped to nothing", pool,
                         [c[2] for c in DET_CLAMP], [c[0] for c in DET_CLAMP], _check_det_clamp))
    tiny = rng.integers(0, 256, (3, 13, 13)).astype(np.uint8)
    cases.append(DetCase("tiny13", "13 x 13: a single valid position", tiny, [0, 1, 2, 0, 1, 2, 2],
                         [[0, 0, 13, 13], [6, 6, 7, 7], [-9, -9, 40, 40], [7, 7, 13, 13], [6, 6, 6, 6], [6, 0, 13, 7], [0, 6, 7, 13]],
                         _check_det_tiny13))
    tiny = rng.integers(0, 256, (4, 13, 14)).astype(np.uint8)
    cases.append(DetCase("tiny14", "14 x 13: two valid positions", tiny, [0, 1, 2, 3, 3, 3],
                         [[0, 0, 14, 13]] * 4 + [[7, 6, 8, 7], [6, 6, 7, 7]], _check_det_tiny14))
    cases.append(DetCase("ties", "equal maxima inside a tile, across tiles, first maximum in a later tile", pool,
                         [c[1] for c in DET_TIES], [c[0] for c in DET_TIES], _check_det_ties))
    idx, regions = _det_structure_jobs()
    cases.append(DetCase("structure", "rank-one and flat structure (eigenvalue exactly 0), the largest sums", pool, idx, regions,
                         _check_det_structure))
    # about 300 jobs in one call, everything above that lives on the pool
    idx, regions = [], []
    for c in (cases[0], cases[1], cases[4], cases[5]):
        idx += list(c.idx); regions += [list(r) for r in c.regions]
    for t in range(300 - len(idx)):
        us, vs = int(rng.integers(-10, DW - 60)), int(rng.integers(-10, DH - 40))
        regions.append([us, vs, us + 80, vs + 60]); idx.append(int(rng.integers(0, len(pool))))
    cases.append(DetCase("many", "300 jobs over ten images in one call", pool, idx, regions, _check_det_many))
    return cases


# ----- multi-ellipse search --------------------------------------------------------------------------------------------
MW, MH = 176, 72         # a box of 129 columns fits; period 5 x 6
ME_WIDTHS = [1, 15, 17, 31, 33, 63, 65, 129, 16, 32, 64]
ME_HEIGHTS = [1, 3, 5, 7, 11, 13]


def _ell(nu, nv, vc=36, uc=88):
    """An axis-aligned ellipse whose clipped box is nu x nv: an odd size from the half-axis, an even one from clipping at the
    left / top border (the centre moves there)."""
    hw, cu = ((nu - 1) // 2, uc + 0.4) if nu % 2 else (nu // 2, nu // 2 + 4 + 0.4)
    hh, cv = ((nv - 1) // 2, vc + 0.6) if nv % 2 else (nv // 2, nv // 2 + 4 + 0.6)
    return _diag(hw, hh) + (cu, cv)


def _me_width_jobs():
    """[(name, [(nu, nv)], vc rows, form)]"""
    hs = ME_HEIGHTS
    same = [(w, hs[k % 6]) for k, w in enumerate(ME_WIDTHS) for _ in (0, 1)]
    pairs = [(15, 33), (33, 15), (31, 65), (65, 31), (1, 129), (129, 1), (16, 64), (64, 16), (32, 63), (63, 32), (17, 33), (33, 17),
             (15, 31), (31, 15), (16, 17), (17, 32), (33, 129), (129, 65)]
    mixed = [(w, hs[(k + j) % 6]) for k, p in enumerate(pairs) for j, w in enumerate(p)]
    jobs = [("same pairs", same, [36], "lds"), ("mixed pairs", mixed, [36], "lds")]
    jobs += [("single %d" % w, [(w, hs[k % 6])], [36], "lds") for k, w in enumerate(ME_WIDTHS)]
    jobs += [("odd count", [(31, 13), (17, 7), (15, 11)], [36], "lds"), ("odd count wide", [(65, 5), (33, 13), (129, 3)], [36], "lds"),
             ("odd count mixed", [(15, 3), (33, 7), (16, 11), (64, 1), (1, 13)], [36], "lds"),
             ("even heights", [(15, 2), (33, 2), (31, 4), (65, 6), (129, 2), (16, 2)], [36], "lds"),
             ("same pairs, two rows", same, [20, 52], "big"), ("mixed pairs, two rows", mixed, [22, 49], "big")]
    return jobs


def _check_me_widths(case, want):
    seen = {}
    for j, (name, sizes, rows, form) in enumerate(_me_width_jobs()):
        boxes, union = case.boxes(j)
        assert [(b[3], b[5]) for b in boxes] == sizes * len(rows), (name, boxes)
        assert me_form(boxes, union) == form, (name, union)
        for e, b in enumerate(boxes):
            if form == "big":
                seen.setdefault(b[3], set()).add("big")
                continue
            seen.setdefault(b[3], set()).add("half" if me_half_mode(boxes, e) else "whole")
            if len(boxes) == 1:
                seen[b[3]].add("alone")
            if len(boxes) % 2 and e == len(boxes) - 1:
                seen[b[3]].add("unpaired")
            seen[b[3]].add("first" if e % 2 == 0 else "second")
    for w in ME_WIDTHS:
        assert {"big", "alone", "first", "second", "whole"} <= seen[w] and ("half" in seen[w]) == (w <= ME_HALF_COLS), (w, seen[w])
    heights = {b[5] for j in range(len(case.counts)) for b in case.boxes(j)[0]}
    assert {1, 2, 3, 5, 6, 7, 11, 13} <= heights


ME_TIES = [  # ellipses of a job [(nu, nv)], rows, carrier ellipse, kinds its ties must straddle
    ([(31, 13), (31, 13)], [36], 0, {"same_lane", "cross_lane"}),
    ([(31, 13), (31, 13)], [36], 1, {"same_lane", "cross_lane"}),
    ([(15, 13), (17, 13)], [36], 0, {"same_lane", "cross_lane"}),        # half a wavefront, two row lanes per column
    ([(65, 13), (15, 13)], [36], 0, {"same_lane", "cross_lane", "cross_half"}),
    ([(65, 13), (15, 13)], [36], 1, {"cross_lane", "cross_half"}),       # a narrow box walked by the whole wavefront: rows across halves
    ([(63, 11)], [36], 0, {"cross_half"}),
    ([(129, 13)], [36], 0, {"cross_half", "cross_block", "same_lane"}),
    ([(129, 13), (31, 13)], [20, 52], 0, {"cross_part", "cross_block", "cross_half"}),
    ([(129, 13), (31, 13)], [20, 52], 3, {"cross_part", "cross_lane"}),
]


def _check_me_ties(case, want):
    for j, (sizes, rows, e, kinds) in enumerate(ME_TIES):
        boxes, union = case.boxes(j)
        assert [(b[3], b[5]) for b in boxes] == sizes * len(rows)
        assert (me_form(boxes, union) == "big") == ("cross_part" in kinds)
        ties = case.ties(j, e, want)
        res = want[j][0]
        assert len(ties) >= 2 and res[e, 0] == 1, (j, e, ties)
        # the LAST of them in scan order is the oracle's answer
        assert (boxes[e][0] + boxes[e][2] + ties[-1][0], boxes[e][1] + boxes[e][4] + ties[-1][1]) == (res[e, 1], res[e, 2])
        assert kinds <= case.tie_kinds(j, e, want), (j, e, kinds, case.tie_kinds(j, e, want))
    # a frame-sized ellipse: its ties straddle the sixteen row parts
    j = len(ME_TIES)
    boxes, union = case.boxes(j)
    assert me_form(boxes, union) == "big" and boxes[0][3] == MW - 10 and boxes[0][5] == MH - 10
    assert {"cross_part", "cross_block", "cross_half", "cross_lane"} <= case.tie_kinds(j, 0, want)


def _check_me_counts(case, want):
    assert list(case.counts) == [255, 256, 257]
    for j in range(3):
        boxes, union = case.boxes(j)
        assert union[2] * union[3] <= ME_CAP and (union[2] + 10) * (union[3] + 10) <= ME_IMG_CAP, union
        assert case.form(j) == ("big" if j == 2 else "lds")
        assert union[3] < ME_BIG_SLICES and all(b[5] < ME_BIG_PARTS for b in boxes)     # fewer rows than slices / than parts
        assert want[j][0][:, 0].all()                          # every ellipse finds an exact copy
        assert all(len(case.ties(j, e, want)) >= 2 for e in (0, 100, int(case.counts[j]) - 1))


def _check_me_area(case, want):
    areas = []
    for j in range(len(case.counts)):
        boxes, union = case.boxes(j)
        assert all((b[3], b[5]) == (33, 31) for b in boxes)
        areas.append((union[2], union[3]))
    assert areas[0] == (64, 32) and 64 * 32 == ME_CAP and case.form(0) == "lds"
    assert ME_CAP < areas[1][0] * areas[1][1] <= ME_CAP + 64 and case.form(1) == "big"
    assert all(w[0][:, 0].all() for w in want)


def _check_me_thin(case, want):
    boxes, union = case.boxes(0)
    assert all((b[3], b[5]) == (19, 5) for b in boxes)
    assert union[2] * union[3] <= ME_CAP and (union[2] + 10) * (union[3] + 10) > ME_IMG_CAP and case.form(0) == "memory", union
    assert want[0][0][:, 0].all()


def _check_me_novalid(case, want):
    forms = [case.form(j) for j in range(len(case.counts))]
    assert forms == ["lds", "none", "lds", "lds", "big", "big", "none", "lds"], forms
    for j, dead in ((1, [0, 1, 2]), (3, [0, 2, 4]), (4, [1, 3]), (5, list(range(257))), (6, [0])):
        boxes, _ = case.boxes(j)
        for e, b in enumerate(boxes):
            assert (b[3] <= 0 or b[5] <= 0) == (e in dead), (j, e, b)
            if e in dead:
                assert list(want[j][0][e]) == [0, 0, 0] and want[j][1][e] == 1000000.0
            else:
                assert want[j][0][e, 0] == 1


def _check_me_bigjobs(case, want):
    assert len(case.counts) == 12 and [case.form(j) for j in range(12)].count("big") == 11 > ME_BIG_GRID_Y
    assert case.counts.max() > ME_BIG_GRID_X and case.counts.max() <= ME_ELL_CAP
    assert all(w[0][:, 0].all() for w in want)


def _check_me_borders(case, want, form):
    j = len(case.counts) - 1
    boxes, (x0, y0, bw, bh) = case.boxes(j)
    assert case.idx[j] == len(case.images) - 1
    assert (x0 - 5, y0 - 5, x0 + bw + 5, y0 + bh + 5) == (0, 0, case.W, case.H) and case.form(j) == form
    assert want[j][0][:, 0].all()


def _check_me_trunc(case, want):
    boxes, _ = case.boxes(0)
    ce = case.ce[case.sl(0)]
    assert [(b[0], b[1]) for b in boxes] == [(0, 0), (0, 30), (-3, 30), (40, 0), (40, 30), (-1, -1)]
    assert all(int(np.floor(c[0])) != b[0] or int(np.floor(c[1])) != b[1] for c, b in list(zip(ce, boxes))[:4])   # truncation, not floor
    assert all(b[3] > 0 and b[5] > 0 for b in boxes)


def _check_me_lowsigma(case, want, oa):
    img, patch = case.images[0], case.patches[0].reshape(11, 11)
    _, _, sd_flat = oa.correlate2_warning(patch, img, 20 - 5, 20 - 5)
    base, _, sd_ten = oa.correlate2_warning(patch, img, 60 - 5, 40 - 5)
    assert sd_flat == 0.0 and abs(sd_ten - 10.0) < 1e-9, (sd_flat, sd_ten)
    assert [case.form(j) for j in range(4)] == ["lds", "lds", "lds", "big"]
    assert want[0][1][0] >= 5.0 and want[0][0][0, 0] == 0                      # flat block: the penalty on every position
    # the window at the threshold, alone in its ellipse: the score with or without the penalty, the oracle decides which
    boxes, _ = case.boxes(1)
    assert (boxes[0][3], boxes[0][5], boxes[0][0], boxes[0][1]) == (1, 1, 60, 40)
    assert want[1][1][0] == (base + 5.0 if sd_ten < 10.0 else base)
    assert want[2][0][0, 0] == 1                                                # the textured part still finds its copy
    assert (want[3][0] == np.concatenate([want[0][0], want[1][0], want[2][0]])).all()


def _check_me_wide(case, want, band):
    boxes, (x0, y0, bw, bh) = case.boxes(0)
    assert case.form(0) == "big" and bw == case.W - 10
    got = ME_BAND_BYTES // (bw + 10) - 10
    assert (got == band) if band else (got <= 0), got
    assert want[0][0][:, 0].all() and "cross_block" in case.tie_kinds(0, 0, want)


def multi_ellipse_cases(oa):
    rng = np.random.default_rng(4321)
    cases = []
    img = periodic(rng, MH, MW, 6, 5)
    tpl = _cut(img, 60, 30)

    jobs = [(0, tpl, [_ell(nu, nv, vc) for vc in rows for nu, nv in sizes]) for _, sizes, rows, _ in _me_width_jobs()]
    cases.append(MeCase("widths", "box widths 1 .. 129 at 16/17, 32/33, 64/65 as both members of a pair, mixed, alone, unpaired; "
                        "heights 1, 2, 3, ...; both forms", img[None], jobs, _check_me_widths))

    jobs = [(0, tpl, [_ell(nu, nv, vc) for vc in rows for nu, nv in sizes]) for sizes, rows, _, _ in ME_TIES]
    jobs.append((0, tpl, [_sinv(20000.0, 100.0, 20000.0) + (88.5, 36.5)]))
    cases.append(MeCase("ties", "equal minima inside a lane, across lanes, halves, column blocks and the 16 row parts", img[None], jobs,
                        _check_me_ties))

    small = periodic(rng, 72, 96, 6, 5)
    stpl = _cut(small, 40, 30)
    jobs = []
    for n in (255, 256, 257):
        jobs.append((0, stpl, [_diag(7 + (k % 2), 5) + (40.3 + (k % 19), 30.7 + (k // 19) % 11) for k in range(n)]))
    cases.append(MeCase("counts", "255, 256, 257 ellipses over a small union: kMeEllCap", small[None], jobs, _check_me_counts))

    jobs = [(0, stpl, [_diag(16, 15) + (30.5, 30.5), _diag(16, 15) + (61.5, 30.5 + dy)]) for dy in (1, 2)]
    cases.append(MeCase("area", "union box of exactly kMeCap positions, and just beyond", small[None], jobs, _check_me_area))

    thin = periodic(rng, 40, 480, 6, 5)
    jobs = [(0, _cut(thin, 200, 20), [_sinv(9.0, 0.1, 0.5) + (30.2 + 7.3 * k, 20.4) for k in range(54)])]
    cases.append(MeCase("thin", "area <= kMeCap but the image tile does not fit: scored from memory", thin[None], jobs, _check_me_thin))

    off = _diag(7, 5) + (-50.0, 30.0)                          # clipped to nothing
    below = _diag(7, 5) + (40.0, 500.0)
    ok = [_diag(8, 6) + (40.3 + 3 * k, 30.7) for k in range(4)]
    huge = _sinv(20000.0, 0.0, 20000.0) + (48.5, 36.5)
    jobs = [(0, stpl, ok), (0, stpl, [off, below, off]), (0, stpl, ok[:2]), (0, stpl, [off, ok[0], below, ok[1], off]),
            (0, stpl, [huge, off, ok[0], below]), (0, stpl, [off] * 257), (0, stpl, [below]), (0, stpl, ok[1:])]
    cases.append(MeCase("novalid", "ellipses clipped to nothing: alone in a job in mid-batch, mixed, in the many-workgroup form",
                        small[None], jobs, _check_me_novalid))

    imgs = np.stack([periodic(rng, 72, 96, 6, 5) for _ in range(3)])
    jobs = []
    for k in range(12):
        i = k % 3
        t = _cut(imgs[i], 40 + k, 30)
        if k == 5:
            jobs.append((i, t, ok))
        elif k == 7:
            jobs.append((i, t, [_sinv(2000.0 + 10 * e, 30.0, 1500.0 + 7 * e) + (20.2 + 0.4 * e, 30.0 + 0.1 * e) for e in range(130)]))
        else:
            jobs.append((i, t, [_sinv(20000.0 - 900 * k, 50.0 * k, 9000.0 + 800 * k) + (48.5 + k, 36.5 - k) for _ in range(1 + k % 3)]))
    cases.append(MeCase("bigjobs", "eleven jobs beyond kMeCap in one call (kMeBigGridY = 8), one with 130 ellipses (kMeBigGridX = 128)",
                        imgs, jobs, _check_me_bigjobs))

    jobs = [(0, _cut(imgs[0], 30, 30), ok), (2, _cut(imgs[2], 50, 40), [huge, _sinv(30000.0, -200.0, 25000.0) + (10.0, 60.0)])]
    cases.append(MeCase("borders big", "many-workgroup union touching all four borders of the last image", imgs, jobs,
                        lambda c, w: _check_me_borders(c, w, "big")))
    imgs60 = np.stack([periodic(rng, 40, 60, 6, 5) for _ in range(2)])
    jobs = [(0, _cut(imgs60[0], 20, 20), [_diag(8, 6) + (25.0, 20.0)]),
            (1, _cut(imgs60[1], 33, 17), [_sinv(5000.0, 10.0, 5000.0) + (30.0, 20.0), _diag(8, 6) + (25.0, 20.0)])]
    cases.append(MeCase("borders one", "one-workgroup union touching all four borders of the last image", imgs60, jobs,
                        lambda c, w: _check_me_borders(c, w, "lds")))
    for w in (11, 12):
        tiny = rng.integers(0, 256, (2, 11, w)).astype(np.uint8)
        jobs = [(0, tiny[0, :, :11], [_diag(8, 6) + (5.5, 5.5)]),
                (1, tiny[1, :, w - 11:], [_sinv(5000.0, 10.0, 5000.0) + (3.0, 7.0), _diag(0, 0) + (w - 6 + 0.2, 5.9), _diag(2, 2) + (w - 6 + 0.5, 5.0)])]
        cases.append(MeCase("borders %dx11" % w, "an image of %d x 11: %d position(s)" % (w, w - 10), tiny, jobs,
                            lambda c, w_: _check_me_borders(c, w_, "lds")))

    jobs = [(0, stpl, [_diag(8, 6) + c for c in ((-0.7, -0.2), (-0.999, 30.9), (-3.9, 30.2), (40.99, -0.5), (40.7, 30.3), (-1.5, -1.01))])]
    cases.append(MeCase("truncation", "negative and fractional centres: int(-0.7) == 0", small[None], jobs, _check_me_trunc))

    low = periodic(rng, 72, 96, 6, 5)
    low[5:36, 5:36] = 128                                       # a flat block
    low[35:46, 55:66] = rng.permutation(np.array([60] * 21 + [61] * 50 + [81] * 50, dtype=np.uint8)).reshape(11, 11)   # sigma 10
    ells = [_diag(8, 6) + (20.5, 20.5), _diag(0, 0) + (60.2, 40.2), _diag(8, 6) + (58.5, 41.5), _diag(8, 6) + (80.5, 55.5)]
    ltpl = _cut(low, 80, 60)
    jobs = [(0, ltpl, ells[:1]), (0, ltpl, ells[1:3]), (0, ltpl, ells[3:]), (0, ltpl, ells)]
    cases.append(MeCase("lowsigma", "a flat block (sigma 0) and a window whose sigma is 10 up to rounding", low[None], jobs,
                        lambda c, w: _check_me_lowsigma(c, w, oa)))

    for W, band in ((1480, 1), (1600, 0)):
        wide = periodic(rng, 24, W, 6, 5)
        jobs = [(0, _cut(wide, 905, 11), [_sinv(80000.0 + 9000 * k, 40.0 * k, 900.0 + 50 * k) + (W / 2 + 3.3 * k, 11.5 + 0.3 * k) for k in range(5)])]
        cases.append(MeCase("wide %d" % W, "a union %d columns wide: an LDS band of %d row(s) in k_me_big_scores" % (W - 10, band),
                            wide[None], jobs, lambda c, w, band=band: _check_me_wide(c, w, band)))
    return cases


DETECTOR_CASE_NAMES = ("sizes", "clamp", "tiny13", "tiny14", "ties", "structure", "many")
MULTI_ELLIPSE_CASE_NAMES = ("widths", "ties", "counts", "area", "thin", "novalid", "bigjobs", "borders big", "borders one", "borders 11x11",
                            "borders 12x11", "truncation", "lowsigma", "wide 1480", "wide 1600")
_CACHE = {}


def all_detector_cases():
    if "det" not in _CACHE:
        _CACHE["det"] = detector_cases()
        assert tuple(c.name for c in _CACHE["det"]) == DETECTOR_CASE_NAMES
    return _CACHE["det"]


def all_multi_ellipse_cases(oa):
    if "me" not in _CACHE:
        _CACHE["me"] = multi_ellipse_cases(oa)
        assert tuple(c.name for c in _CACHE["me"]) == MULTI_ELLIPSE_CASE_NAMES
    return _CACHE["me"]


def detector_case(name):
    return all_detector_cases()[DETECTOR_CASE_NAMES.index(name)]


def multi_ellipse_case(name, oa):
    return all_multi_ellipse_cases(oa)[MULTI_ELLIPSE_CASE_NAMES.index(name)]

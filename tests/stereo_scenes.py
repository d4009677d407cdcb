"""Planted stereo scenes for Frame::ComputeStereoMatches (reference src/Frame.cc:880-1176): images, hand-made keypoints and
descriptors, and the line of the function each planted keypoint is meant to leave at (`reason`, codes of stereo_model; -1 = not
planted, only compared).  Nothing here calls the model, the oracle's stereo match or the library: the intent is stated from the
reference text, the tests then ask model, oracle and kernels for it.

Coordinates.  A keypoint lives in the coordinates of mvImagePyramid[0]: on a fork handle that is the image with 19 reflected
pixels around it (view = image + 19), on an ORBX_PYRAMID_UPSTREAM handle the image itself.

The function's only outputs are mvuRight and mvDepth, so a decision is visible from outside only where one side of it ends in a
kept match: every "passing" side below is planted to end as MATCHED.

Two kinds of pixels:
 * cols: L(x, y) = G(x) + e, R(x, y) = G(x + d) + e' with G seeded per column and e, e' in 0..3.  Every left keypoint has its match
   d columns to the left in the right image, on every row and (up to the resize) at every octave; the SADs are all about the same, so
   the median cut keeps them all.  Near the left and right edge G is periodic with period 2 d and symmetric about the edge
   column, which is what makes the 19 reflected pixels of a fork handle's level 0 carry the same shift.  Bounds, gates, octave
   windows and row bands are planted on these.
 * noise: independent seeded noise in both eyes.  A planted match copies the 11 x 17 block around the left keypoint into the right
   image `d` columns to the left and raises k non-centre pixels of the right patch by a: the SAD at the true shift is exactly
   k * a, every other shift compares unrelated noise (thousands).  `sym` mirrors the block about its centre column first, which
   makes SAD(+1) == SAD(-1), deltaR == 0 and the disparity an exact number.
"""
import functools

import numpy as np

import stereo_model as sm
import upstream_model as um

KP = um.KP
EDGE = um.EDGE
f32 = np.float32
MODES = ("fork", "upstream")
SIZES = ((160, 120), (96, 64))


class Scene:
    pass


class Builder:
    def __init__(self, name, mode, w, h, nlevels=3, factor=1.2, mb=0.5, mbf=10.0, seed=1, cols=0):
        self.name, self.mode, self.w, self.h, self.nlevels, self.factor = name, mode, w, h, nlevels, factor
        self.mb, self.mbf = mb, mbf
        self.maxD = f32(f32(mbf) / f32(mb))
        self.rng = np.random.default_rng(seed)
        self.scale, self.inv, _ = um.tables(100, factor, nlevels)
        pad = 2 * EDGE if mode == "fork" else 0
        self.off = EDGE if mode == "fork" else 0
        self.W = [sw + pad for sw, sh in um.level_sizes(w, h, self.inv)]      # mvImagePyramid[l].cols / .rows
        self.H = [sh + pad for sw, sh in um.level_sizes(w, h, self.inv)]
        self.nrows0 = self.H[0]
        if cols:
            self.imgL, self.imgR = self.col_texture(cols, h)
        else:
            self.imgL = self.rng.integers(60, 181, (h, w)).astype(np.uint8)
            self.imgR = self.rng.integers(60, 181, (h, w)).astype(np.uint8)
        self.cols = cols
        self.kl, self.kr, self.dl, self.dr, self.reason = [], [], [], [], []
        self.blocks = []         # (row0, row1, col0, col1) in image coordinates, inclusive: pixels a planted match owns
        self.band, self.cursor = 0, 0

    def col_texture(self, d, nrows):
        """(L, R) of `nrows` rows: R(x) = L(x + d), also through the reflected border of a fork handle's level 0"""
        w = self.w
        G = self.rng.integers(60, 181, w + 2 * EDGE + d + 1)            # G over the padded columns x' = x + 19, and d beyond
        fold = lambda t: abs((t + d) % (2 * d) - d)                     # distance to the nearest multiple of 2 d
        for edge in (EDGE, EDGE + w - 1):                               # symmetric about `edge` and about `edge + d`
            Hs = self.rng.integers(60, 181, d + 1)
            for x in range(edge - EDGE, edge + EDGE + d + 1):
                G[x] = Hs[fold(x - edge)]
        L = G[None, EDGE:EDGE + w] + self.rng.integers(0, 4, (nrows, w))
        R = G[None, EDGE + d:EDGE + d + w] + self.rng.integers(0, 4, (nrows, w))
        return L.astype(np.uint8), R.astype(np.uint8)

    # ---- keypoints
    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def flipped(self, d, nbits):
        bits = np.unpackbits(d)
        bits[self.rng.choice(256, nbits, replace=False)] ^= 1
        return np.packbits(bits)

    def right(self, x, y, octave, d):
        self.kr.append((f32(x), f32(y), f32(31), f32(0), f32(1), octave, -1))
        self.dr.append(d)
        return len(self.kr) - 1

    def left(self, x, y, octave, d, reason):
        self.kl.append((f32(x), f32(y), f32(31), f32(0), f32(1), octave, -1))
        self.dl.append(d)
        self.reason.append(reason)
        return len(self.kl) - 1

    def pair(self, xl, yl, xr, yr, reason, ol=0, orr=None, bits=0):
        """one left and one right keypoint that differ in `bits` descriptor bits"""
        d = self.desc()
        self.right(xr, yr, ol if orr is None else orr, d)
        return self.left(xl, yl, ol, self.flipped(d, bits), reason)

    def coord(self, level, c):
        """keypoint coordinate whose round(c * mvInvScaleFactors[level]) (:1031-1033) is the level pixel `c`"""
        v = f32(f32(c) * self.scale[level])
        assert sm.c_round(f32(v * self.inv[level])) == c, (level, c)
        return v

    # ---- planted matches (noise images, octave 0)
    def alloc(self, d, extra=0):
        """image coordinates of a free slot for a match of integer shift d (`extra` more columns to its left)"""
        while True:
            iy = 6 + 12 * self.band
            assert iy + 5 < self.h, "scene %s is full" % self.name
            ix = self.cursor + 15 + d + extra
            end = max(ix + 8, ix - d + 16)
            if end < self.w:
                self.cursor = end + 1
                return ix, iy
            self.band, self.cursor = self.band + 1, 0

    def plant(self, ix, iy, d, k, a, sym=False):
        """the match itself: after this the SAD of left patch (ix, iy) against right patch (ix - d, iy) is k * a"""
        L, R = self.imgL, self.imgR
        assert 8 <= ix - d and ix + 8 < self.w and 5 <= iy and iy + 5 < self.h and a <= 60 and 0 <= k <= 100
        if sym:
            assert k % 2 == 0
            L[iy - 5:iy + 6, ix + 1:ix + 9] = L[iy - 5:iy + 6, ix - 8:ix][:, ::-1]
        R[iy - 5:iy + 6, ix - d - 8:ix - d + 9] = L[iy - 5:iy + 6, ix - 8:ix + 9]
        # raised pixels: rows from the top, columns +-j pairwise (symmetric about the centre column, never the centre pixel)
        cells = [(dy, s * j) for dy in (-5, -4, -3, -2, -1, 1, 2, 3, 4, 5) for j in (1, 2, 3, 4, 5) for s in (1, -1)][:k]
        for dy, dx in cells:
            v = int(R[iy + dy, ix - d + dx]) + a
            assert v <= 255, "a raised pixel saturates"
            R[iy + dy, ix - d + dx] = v
        # the pixels this match owns: its left block, and every right column a window of +-10 about uR0 = true +-5 can touch
        self.blocks.append((iy - 5, iy + 5, ix - 8, ix + 8, "L"))
        self.blocks.append((iy - 5, iy + 5, ix - d - 15, ix - d + 15, "R"))

    def match(self, d, sad_ka, reason, sym=False, bits=0, duL=0.0, uR_off=0, copies=1, extra=0, at=None):
        """planted match of shift d and SAD k * a; the right keypoint sits uR_off columns right of the true match (bestincR =
        -uR_off), both keypoints duL right of the pixel centre.  `copies` left keypoints share it."""
        k, a = sad_ka
        ix, iy = at if at else self.alloc(d, extra)
        self.plant(ix, iy, d, k, a, sym)
        vx, vy = ix + self.off, iy + self.off
        dsc = self.desc()
        ir = self.right(f32(vx - d + uR_off + duL), vy, 0, dsc)
        il = [self.left(f32(vx + duL), vy, 0, self.flipped(dsc, bits), reason) for _ in range(copies)]
        return il, ir, (vx, vy)

    def finish(self, cut=None):
        for i, a in enumerate(self.blocks):
            for b in self.blocks[i + 1:]:
                if a[4] == b[4]:
                    assert a[1] < b[0] or b[1] < a[0] or a[3] < b[2] or b[3] < a[2], "planted windows overlap: %s %s" % (a, b)
        s = Scene()
        s.name, s.mode, s.w, s.h, s.nlevels, s.factor, s.mb, s.mbf = (self.name, self.mode, self.w, self.h, self.nlevels,
                                                                      self.factor, self.mb, self.mbf)
        s.imgL, s.imgR = self.imgL, self.imgR
        s.kL = np.array(self.kl, KP) if self.kl else np.zeros(0, KP)
        s.kR = np.array(self.kr, KP) if self.kr else np.zeros(0, KP)
        s.dL = np.array(self.dl, np.uint8).reshape(-1, 32)
        s.dR = np.array(self.dr, np.uint8).reshape(-1, 32)
        s.reason = np.array(self.reason, np.int32)
        s.scale, s.inv, s.W, s.H = self.scale, self.inv, self.W, self.H
        s.cut = cut            # "both": the median cut keeps and drops; "all": it drops every match; None: it drops nothing
        for a in (s.imgL, s.imgR, s.kL, s.kR, s.dL, s.dR, s.reason):
            a.setflags(write=False)
        return s


def ka(sad, even=False):
    """k pixels raised by a with k * a == sad"""
    if sad == 0:
        return 0, 0
    for a in range(55, 0, -1):
        if sad % a == 0 and sad // a <= 100 and not (even and (sad // a) % 2):
            return sad // a, a
    raise ValueError(sad)


# ------------------------------------------------------------------------------------------------------------------ bounds
def bounds(mode, w, h, cols, nlevels=3, factor=1.2, octaves=(0, 1), mbf=10.0):
    """each of y0, y0 + 11 - H, x0, x0 + 11 - W, iniu and W - 1 - endu at -1, 0 and +1 (:1040-1042, :1071-1072), per octave.  On the
    column texture (shift `cols` at level 0, an integer at the octaves used) the passing keypoints match; on noise they are compared
    only, and so are the passing x cases above octave 0 of a fork handle: the reflected border of a RESIZED level does not carry the
    shift.  40 left keypoints on one planted match of SAD 2000 hold the median, so that the cut (:1160-1175) keeps every other
    match whatever its SAD."""
    b = Builder("bounds_%s_%dx%d_%s_%d" % (mode, w, h, "cols" if cols else "noise", nlevels), mode, w, h, nlevels, factor,
                mbf=mbf, seed=11, cols=cols)
    ok = sm.MATCHED if cols else -1
    d0 = cols if cols else 6

    def shift(l):
        """the level-0 shift d0 at level l.  A level is resized from mvImagePyramid[l - 1], which on a fork handle is the PADDED
        level (src/ORBextractor.cc:2166), so there the ratio is not the scale factor"""
        r = float(d0)
        for k in range(1, l + 1):
            r *= (b.W[k] - 2 * b.off) / b.W[k - 1]
        assert not cols or (abs(r - round(r)) < 0.1 and round(r) >= 2), (l, r)
        return int(round(r))

    def add(l, sul, svl, roff, reason):
        """left keypoint at level pixel (sul, svl); the right one `roff` pixels right of the true match (bestincR = -roff)"""
        dl = shift(l)
        xl, yl, xr = b.coord(l, sul), b.coord(l, svl), b.coord(l, sul - dl + roff)
        assert xr <= xl and xr >= xl - b.maxD
        if int(yl) >= b.nrows0:     # F6 comes first: the level-l row scaled back lies past mvImagePyramid[0].rows (:968)
            reason = sm.ROW_CLAMPED
        b.pair(xl, yl, xr, yl, reason, ol=l)

    if cols:
        b.match(d0, ka(2000), sm.MATCHED, copies=40, at=(max(w // 4 - 12, 16 + d0), h // 4))
    for l in octaves:
        W, H = b.W[l], b.H[l]
        dl = shift(l)
        okx = ok if mode == "upstream" or l == 0 else -1
        mx, my = W // 2 + 4, H // 2
        for dlt in (-1, 0, 1):
            add(l, mx, 5 + dlt, 0, sm.Y0_NEG if dlt < 0 else ok)                         # y0 = dlt
            add(l, mx, H - 6 + dlt, 0, sm.Y1_OVER if dlt > 0 else ok)                    # y0 + 11 - H = dlt
            add(l, 5 + dlt, my, dl, sm.X0_NEG if dlt < 0 else sm.INIU_NEG)               # x0 = dlt: uR <= uL forces iniu < 0
            add(l, W - 6 + dlt, my, -4, sm.X1_OVER if dlt > 0 else okx)                  # x0 + 11 - W = dlt
            add(l, 10 + dlt + dl, my, 0, sm.INIU_NEG if dlt < 0 else okx)               # iniu = dlt
            add(l, W - 12 - dlt + dl - min(4, dl), my, min(4, dl), sm.ENDU_OVER if dlt < 0 else okx)   # W - 1 - endu = dlt
    return b.finish()


# ------------------------------------------------------------------------------------------------------------------- gates
def band(b, y, octave):
    """[minr, maxr] of :934-936"""
    r = f32(f32(2.0) * b.scale[octave])
    return int(np.floor(f32(f32(y) - r))), int(np.ceil(f32(f32(y) + r)))


def rows(mode, w, h, octave):
    """row bands (:934-941): right keypoints at y = n, n + 0.25, n + 0.6 of one octave, left keypoints on the first and last row
    of each band and one row outside; bands cut at row 0 and nrows0 - 1; vL at -1, -0.5, nrows0 - 0.5 and nrows0"""
    b = Builder("rows_%s_%dx%d_o%d" % (mode, w, h, octave), mode, w, h, cols=6, seed=12)
    ux = f32(b.W[0] // 2)
    for n, frac in ((15, 0.0), (30, 0.25), (45, 0.6)):
        y = f32(n + frac)
        lo, hi = band(b, y, octave)
        assert (lo, hi) == {0: {0.0: (n - 2, n + 2), 0.25: (n - 2, n + 3), 0.6: (n - 2, n + 3)},
                            1: {0.0: (n - 3, n + 3), 0.25: (n - 3, n + 3), 0.6: (n - 2, n + 3)},      # r = 2.4
                            2: {0.0: (n - 3, n + 3), 0.25: (n - 3, n + 4), 0.6: (n - 3, n + 4)}}[octave][frac]   # r = 2.88
        d = b.desc()
        b.right(ux - 6, y, octave, d)
        for vl, reason in ((lo + 0.5, sm.MATCHED), (hi + 0.5, sm.MATCHED), (lo, sm.MATCHED),
                           (lo - 0.5, sm.NO_CANDIDATE), (hi + 1, sm.NO_CANDIDATE)):
            b.left(ux, f32(vl), octave, d, reason)
    nr = b.nrows0
    d = b.desc()
    b.right(ux - 6, 1.0, 0, d)                       # band -1 .. 3: cut at row 0
    b.left(ux, -1.0, 0, d, sm.ROW_CLAMPED)
    b.left(ux, -0.5, 0, d, sm.Y0_NEG)                # row (int)-0.5 = 0 has the candidate; round(-0.5) = -1 fails :1041
    b.left(ux, 3.5, 0, d, sm.Y0_NEG)
    b.left(ux, 4.0, 0, d, sm.NO_CANDIDATE)
    d = b.desc()
    b.right(ux - 6, nr - 2.0, 0, d)                  # band nrows0 - 4 .. nrows0: cut at row nrows0 - 1
    b.left(ux, nr - 0.5, 0, d, sm.Y1_OVER)           # row nrows0 - 1; round gives nrows0
    b.left(ux, float(nr), 0, d, sm.ROW_CLAMPED)
    b.left(ux, nr - 4.5, 0, d, sm.NO_CANDIDATE)
    b.left(ux, nr - 4.0, 0, d, sm.Y1_OVER)
    return b.finish()


def gates(mode, w, h):
    """uR on minU and maxU (:1005), maxU < 0 (:977), descriptor distance 74 / 75 / 99 / 100 (:1012, :1022).  Shift 4 and maxD = 8:
    a right keypoint on maxU has bestincR = -4, one on minU +4."""
    b = Builder("gates_%s_%dx%d" % (mode, w, h), mode, w, h, mb=0.5, mbf=4.0, cols=4, seed=13)
    assert b.maxD == 8
    ux, vy = f32(b.W[0] // 2 + 12), f32(b.H[0] // 2)
    ok, no = sm.MATCHED, sm.ORB_DIST
    for frac in (0.0, 0.3, 0.7):
        ul = f32(ux + frac)
        minU = f32(ul - b.maxD)
        b.pair(ul, vy, minU, vy, ok)                                         # uR == minU
        b.pair(ul, vy, np.nextafter(minU, f32(-1e9)), vy, no)                # one ulp below
        b.pair(ul, vy, ul, vy, ok)                                           # uR == maxU
        b.pair(ul, vy, np.nextafter(ul, f32(1e9)), vy, no)                   # one ulp above
    b.pair(-0.5, vy, -0.5, vy, sm.MAXU_NEG)
    b.pair(0.0, vy, 0.0, vy, sm.X0_NEG)                                      # maxU == 0 is searched
    for bits, reason in ((74, ok), (75, no), (99, no), (100, no), (0, ok)):
        b.pair(ux, vy, ux - 4, vy, reason, bits=bits)
    # a candidate at 99 does not stop a later one at 74 (bestDist starts at TH_HIGH and only falls)
    d = b.desc()
    b.right(ux - 4, vy, 0, b.flipped(d, 99))
    b.right(ux - 4, vy, 0, b.flipped(d, 74))
    b.left(ux, vy, 0, d, ok)
    return b.finish()


def octaves(mode, w, h, ol):
    """the octave window (:998) around left octave `ol`: right keypoints at every octave, the same place"""
    b = Builder("octaves_%s_%dx%d_o%d" % (mode, w, h, ol), mode, w, h, cols=6, seed=19)
    ux, vy = f32(b.W[0] // 2), f32(b.H[0] // 2)
    for orr in range(b.nlevels):
        b.pair(ux, vy, ux - 6, vy, sm.MATCHED if abs(orr - ol) <= 1 else sm.ORB_DIST, ol=ol, orr=orr)
    return b.finish()


# ------------------------------------------------------------------------------------------------------- ties, descriptors
def ties(mode, w, h):
    """equal-distance candidates: the smallest iR wins (:1012 is a strict '<' over ascending iR).  Only the winner's columns hold
    the planted match; the decoys sit on unrelated noise 32 columns to the left, with smaller y (a table filled in order of y, or in
    any order, still has to return the smallest index)."""
    b = Builder("ties_%s_%dx%d" % (mode, w, h), mode, w, h, mbf=40.0, seed=14)      # maxD = 80: the decoys are inside the gate
    sad = ka(40)
    for ndecoy in (1, 2):
        il, ir, (vx, vy) = b.match(4, sad, sm.MATCHED, extra=32 * ndecoy)
        b.kr[ir] = (b.kr[ir][0], f32(vy + 1),) + b.kr[ir][2:]
        for j in range(ndecoy):
            assert vx - 4 - 32 * (j + 1) >= vx - b.maxD
            b.right(f32(vx - 4 - 32 * (j + 1)), f32(vy - 1 - 0.5 * j), 0, b.dr[ir])
    # a smaller distance at a larger index wins over a larger distance at a smaller index
    ix, iy = b.alloc(4, 32)
    d = b.desc()
    b.right(f32(ix + b.off - 4 - 32), iy + b.off, 0, b.flipped(d, 11))
    b.plant(ix, iy, 4, *sad)
    b.right(f32(ix + b.off - 4), iy + b.off, 0, b.flipped(d, 10))
    b.left(f32(ix + b.off), iy + b.off, 0, d, sm.MATCHED)
    b.match(4, sad, sm.MATCHED, bits=74)
    b.match(4, sad, sm.ORB_DIST, bits=75)
    return b.finish()


# --------------------------------------------------------------------------------------------------------------- disparity
def disparity(mode, w, h):
    """maxD = 12 exactly; symmetric blocks make deltaR 0 and the disparity the planted number (:1132-1142)"""
    b = Builder("disparity_%s_%dx%d" % (mode, w, h), mode, w, h, mb=0.5, mbf=6.0, seed=15)
    assert b.maxD == 12
    sad = ka(40, even=True)
    for _ in range(2):
        b.match(0, sad, sm.CLAMPED, sym=True)                        # disparity == 0: 0.01, bestuR = uL - 0.01 through double
    b.match(0, sad, sm.DISPARITY_RANGE, sym=True, duL=-0.25)         # disparity = -0.25
    b.match(0, sad, sm.MATCHED, sym=True, duL=0.25)                  # disparity = +0.25
    b.match(11, sad, sm.MATCHED, sym=True)                           # maxD - 1
    b.match(11, sad, sm.MATCHED, sym=True, uR_off=-1)                # uR == minU, bestincR = +1
    b.match(12, sad, sm.DISPARITY_RANGE, sym=True)                   # maxD, uR == minU
    b.match(13, sad, sm.DISPARITY_RANGE, sym=True, uR_off=2)         # maxD + 1 through bestincR = -2... uR inside the gate
    b.match(6, sad, sm.BESTINC_END, uR_off=5)                        # bestincR = -5
    b.match(6, sad, sm.MATCHED, uR_off=4)                            # -4
    b.match(6, sad, sm.MATCHED, uR_off=-4)                           # +4
    b.match(6, sad, sm.BESTINC_END, uR_off=-5)                       # +5
    return b.finish()


# ------------------------------------------------------------------------------------------------------------------ median
# name -> (SADs in left-keypoint order, copies of each, what the cut does).  1.5f * 1.4f is 2.0999999f: the threshold of median 30
# is 62.999996 (62 stays, 63 goes), that of median 40 rounds to 84.0 exactly (83 stays, 84 goes).
MEDIAN_SETS = {
    "odd": ([200, 10, 63, 30, 62, 20, 70], 1, "both"),               # 7 matches, rank 3: median 62 -> 130.2
    "floor_ceil": ([63, 10, 30, 62, 20], 1, "both"),                 # median 30: 62 = floor(thDist) stays, 63 = ceil goes
    "even": ([84, 10, 40, 20, 83, 5], 1, "both"),                    # 6 matches, rank 3 (not 2): median 40, 83 stays, 84 goes
    "one": ([50], 1, None),
    "two": ([10, 50], 1, None),                                      # rank 1: the larger one is the median
    "zero_median": ([0, 9, 0, 0, 5], 1, "all"),                      # thDist == 0: nothing is < 0, every match goes
    "high_byte": ([510, 1300, 260, 400, 600, 270, 300], 1, "both"),  # five share the high byte 1; median 400 -> 840
    "many": ([200, 10, 63, 30, 62], 60, "both"),                     # 300 matches: median 62 -> 130.2
}


def median(mode, w, h, which):
    sads, copies, cut = MEDIAN_SETS[which]
    b = Builder("median_%s_%s_%dx%d" % (which, mode, w, h), mode, w, h, seed=16)
    srt = sorted(s for s in sads for _ in range(copies))
    th = f32(f32(f32(1.5) * f32(1.4)) * f32(srt[len(srt) // 2]))     # :1161-1162
    for s in sads:
        b.match(3, ka(s), sm.MATCHED if f32(s) < th else sm.CUT, copies=copies)
    if copies > 1:                # interleave the copies: a, b, c, a, b, c ...
        order = np.arange(len(b.kl)).reshape(len(sads), copies).T.ravel()
        b.kl, b.dl, b.reason = [b.kl[i] for i in order], [b.dl[i] for i in order], [b.reason[i] for i in order]
    return b.finish(cut)


def empty(mode, w, h):
    """counts of 0: no right keypoint at all, so vDistIdx is empty (:1161 would read element 0 of it)"""
    b = Builder("empty_%s_%dx%d" % (mode, w, h), mode, w, h, seed=17)
    il, ir, _ = b.match(3, ka(40), sm.NO_CANDIDATE)
    b.kr, b.dr = [], []
    return b.finish()


# -------------------------------------------------------------------------------------------------------------------- tall
TALL_W, TALL_H = 1360, 2720


def tall():
    """1360 x 2720, 2 levels, fork handle: nrows0 = 2758, about the tallest level 0 the library takes (at most 4095 FAST cells in a
    level and an aspect ratio of at least 0.5 leave no image with more than some 2.8 k rows; 45 x 90 cells here).  Noise with stripes
    of the column texture (shift 6), 45 rows, at the top and the bottom; matches planted down the whole height, bounds and row cuts
    on the stripes, including the last rows."""
    w, h = TALL_W, TALL_H
    b = Builder("tall", "fork", w, h, nlevels=2, seed=18)
    for r0 in (0, h - 45):
        b.imgL[r0:r0 + 45], b.imgR[r0:r0 + 45] = b.col_texture(6, 45)
    nr = b.nrows0
    sads = [40, 10, 200, 62, 30, 63, 20, 70, 25, 35, 45, 2600]   # the median is held at 1000 below: 2100 cuts the last one only
    ys = [60, 300, 700, 1100, 1500, 2000, 2047, 2048, 2300, 2500, h - 52, h - 60]
    for i, (s, iy) in enumerate(zip(sads, ys)):
        b.match(7, ka(s), sm.MATCHED if s < 2100 else sm.CUT, at=(100 + 100 * i, iy))
    b.match(7, ka(1000), sm.MATCHED, copies=40, at=(1300, 1300))
    ux = f32(1000)
    for vl, reason in ((5.0, sm.MATCHED), (4.0, sm.Y0_NEG), (nr - 6.0, sm.MATCHED), (nr - 7.0, sm.MATCHED),
                       (nr - 5.0, sm.Y1_OVER), (nr - 1.0, sm.Y1_OVER), (nr - 0.5, sm.Y1_OVER), (float(nr), sm.ROW_CLAMPED)):
        b.pair(ux, vl, ux - 6, vl, reason)
    d = b.desc()
    b.right(f32(494), nr - 9.0, 0, d)                # band nrows0 - 11 .. nrows0 - 7
    for vl, reason in ((nr - 11.5, sm.NO_CANDIDATE), (nr - 11.0, sm.MATCHED), (nr - 6.5, sm.MATCHED),
                       (nr - 6.0, sm.ORB_DIST)):     # row nrows0 - 6 holds other pairs' keypoints only
        b.left(f32(500), vl, 0, d, reason)
    for x, reason in ((w + 2 * EDGE - 6.0, sm.MATCHED), (w + 2 * EDGE - 5.0, sm.X1_OVER)):
        b.pair(x, nr - 8.0, x - 6 - 4, nr - 8.0, reason)
    return b.finish("both")


def check_planted(s, res):
    """res = stereo_model(...) on the scene: every planted keypoint left at its line, and the cut did what the scene says"""
    n, u, d, sad, reason = res
    planted = s.reason >= 0
    bad = np.nonzero(planted & (reason != s.reason))[0]
    assert len(bad) == 0, [(int(i), sm.NAMES[int(s.reason[i])], sm.NAMES[int(reason[i])]) for i in bad]
    kept = np.isin(reason, (sm.MATCHED, sm.CLAMPED))
    assert n == kept.sum() and ((u >= 0) == kept).all() and ((d > 0) == kept).all() and ((sad >= 0) == (kept | (reason == sm.CUT))).all()
    if s.cut == "both":
        assert kept.any() and (reason == sm.CUT).any()
    elif s.cut == "all":
        assert n == 0 and (reason == sm.CUT).any()
    else:
        assert not (reason == sm.CUT).any()


# ---------------------------------------------------------------------------------------------------------------- registry
def _small():
    out = {}
    for mode in MODES:
        for (w, h) in SIZES:
            for s in ([bounds(mode, w, h, 5 if (mode, w) == ("fork", 96) else 6), bounds(mode, w, h, 0),
                       gates(mode, w, h), ties(mode, w, h),
                       disparity(mode, w, h), empty(mode, w, h)] + [rows(mode, w, h, o) for o in (0, 1, 2)] +
                      [octaves(mode, w, h, o) for o in (0, 1, 2)] +
                      [median(mode, w, h, k) for k in MEDIAN_SETS]):
                out[s.name] = s
    s = bounds("fork", 160, 120, 5, nlevels=4, factor=2.0, octaves=(0, 1), mbf=50.0)   # upstream refuses a 20 x 15 top level
    out[s.name] = s
    return out


@functools.lru_cache(maxsize=None)
def small_scenes():
    return _small()


SMALL_NAMES = sorted(small_scenes())
@functools.lru_cache(maxsize=None)
def tall_scene():
    return tall()


@functools.lru_cache(maxsize=None)
def cpu_pyramids(name):
    """(pyrL, pyrR) of a scene as the extractor builds them (border101 / resize_linear of the oracle's extractor, to which the
    device pyramid is pinned); computed once, shared, read-only"""
    s = tall_scene() if name == "tall" else small_scenes()[name]
    out = []
    for img in (s.imgL, s.imgR):
        M = um.ModelExtractor(100, s.factor, s.nlevels, padded=s.mode == "fork")
        M.compute_pyramid(img)
        lv = [np.ascontiguousarray(a) for a in M.pyr]
        for a in lv:
            a.setflags(write=False)
        out.append(lv)
    return tuple(out)

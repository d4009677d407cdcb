"""ORBextractor::operator() as a Python composition of the oracle's primitives, with one switch: what a pyramid level IS.

`padded=True` restates oracle/orb_oracle.c (compute_pyramid, compute_keypoints, orc_extract): the fork, whose
`mvImagePyramid[level] = temp;` (reference src/ORBextractor.cc:2166) makes a level the padded buffer.  `padded=False` is the
same code without that line, i.e. upstream ORB-SLAM2: a level is the sw x sh view at offset (19, 19) inside `temp`.  Everything
that differs between the two follows from that one choice (`view` below); no other line of the model looks at the switch.

The primitives (border101, resize_linear, fast9_16, distribute_octtree, orc_ic_angle, gaussian_blur7, orc_descriptor,
orc_cv_round_f) are the oracle's, so the padded model must equal OracleExtractor bit for bit (tests/test_upstream_model.py),
which in turn is pinned to the compiled reference.  The upstream switch is pinned to this composition, not to a compiled
upstream tree.
"""
import ctypes as C
import math

import numpy as np

import oracle.orb_oracle as oo

EDGE = 19
PATCH = 31
KP = oo.KP_DTYPE
f32 = np.float32


class UndefinedGeometry(ValueError):
    """the reference is undefined for this image size / level count; .status names the ABI status the library answers with"""

    def __init__(self, status, level, what):
        ValueError.__init__(self, "level %d: %s" % (level, what))
        self.status, self.level = status, level


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _round(v):
    return oo.lib().orc_cv_round_f(C.c_float(float(f32(v))))


def tables(nfeatures, scale_factor, nlevels):
    """mvScaleFactor, mvInvScaleFactor, mnFeaturesPerLevel: the oracle's own (orc_create)"""
    t = oo.OracleExtractor(nfeatures, scale_factor, nlevels).tables()
    return [f32(v) for v in t["scale"]], [f32(v) for v in t["inv_scale"]], [int(v) for v in t["features_per_level"]]


def level_sizes(w, h, inv):
    return [(_round(f32(w) * s), _round(f32(h) * s)) for s in inv]


def level_geometry(cols, rows, nfeat, level=0, strict=True):
    """FAST region, cell grid and quadtree roots of one level whose image is cols x rows (the padded buffer or the view).
    strict: raise on the geometries the reference is undefined for (the library refuses them before any launch)."""
    minB = EDGE - 3
    maxBX, maxBY = cols - EDGE + 3, rows - EDGE + 3
    qt_w, qt_h = maxBX - minB, maxBY - minB
    if strict and (qt_w <= 0 or qt_h <= 0):
        raise UndefinedGeometry("UNSUPPORTED", level, "FAST region %d x %d" % (qt_w, qt_h))
    width, height = f32(qt_w), f32(qt_h)
    ncols, nrows = int(width / f32(30)), int(height / f32(30))
    cells = []
    wcell = hcell = 0
    if ncols > 0 and nrows > 0:
        wcell, hcell = int(np.ceil(width / f32(ncols))), int(np.ceil(height / f32(nrows)))
        for i in range(nrows):
            iniY = minB + i * hcell
            maxY = iniY + hcell + 6
            if iniY >= maxBY - 3:
                continue
            maxY = min(maxY, maxBY)
            for j in range(ncols):
                iniX = minB + j * wcell
                maxX = iniX + wcell + 6
                if iniX >= maxBX - 6:
                    continue
                maxX = min(maxX, maxBX)
                cells.append((iniX, iniY, maxX - iniX, maxY - iniY, j * wcell, i * hcell))
    # DistributeOctTree: nIni = round(width / height) (:1060); C roundf = half away from zero, the ratio is positive
    nini = int(math.floor(float(f32(qt_w) / f32(qt_h)) + 0.5)) if qt_h > 0 and qt_w > 0 else 0
    if strict and nini <= 0:
        raise UndefinedGeometry("BAD_ASPECT", level, "nIni == 0")
    return dict(minB=minB, maxBX=maxBX, maxBY=maxBY, qt_w=qt_w, qt_h=qt_h, ncols=ncols, nrows=nrows, wcell=wcell, hcell=hcell,
                cells=cells, nini=nini, kp_cap=max(nfeat + 3, 4 * nini))


def geometry(w, h, nfeatures=1000, scale_factor=1.2, nlevels=8, padded=False):
    """per-level geometry of a whole handle; kp_total = orbx_max_keypoints"""
    _, inv, per = tables(nfeatures, scale_factor, nlevels)
    out = []
    for l, (sw, sh) in enumerate(level_sizes(w, h, inv)):
        g = level_geometry(sw + 2 * EDGE if padded else sw, sh + 2 * EDGE if padded else sh, per[l], l)
        g["sw"], g["sh"] = sw, sh
        out.append(g)
    return out


class ModelExtractor:
    """same surface as oracle.OracleExtractor (extract, level_image, level_candidates, level_keypoints)"""

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th=20, min_th=7, fp_mode=oo.FP_GCC_FMA, padded=False):
        self.nfeatures, self.nlevels, self.ini_th, self.min_th, self.fp_mode = nfeatures, nlevels, ini_th, min_th, fp_mode
        self.padded = padded
        self.sf, self.inv, self.per = tables(nfeatures, scale_factor, nlevels)
        self.L = oo.lib()

    def view(self, temp, sw, sh):
        """THE switch: mvImagePyramid[level] is `temp` (fork, :2166) or the un-padded window inside it (upstream)"""
        return temp if self.padded else temp[EDGE:EDGE + sh, EDGE:EDGE + sw]

    # -- ComputePyramid
    def compute_pyramid(self, img):
        h, w = img.shape
        self.temp, self.pyr = [], []
        for level, (sw, sh) in enumerate(level_sizes(w, h, self.inv)):
            if sw < 1 or sh < 1:
                raise UndefinedGeometry("UNSUPPORTED", level, "level collapses to zero size")
            if level:
                centre = oo.resize_linear(np.ascontiguousarray(self.pyr[level - 1]), sw, sh)
            else:
                centre = img
            temp = oo.border101(centre, EDGE)
            self.temp.append(temp)
            self.pyr.append(self.view(temp, sw, sh))

    # -- ComputeKeyPointsOctTree
    def compute_keypoints(self):
        self.cand, self.kps = [], []
        geo = [level_geometry(im.shape[1], im.shape[0], self.per[l], l) for l, im in enumerate(self.pyr)]   # raises before any work
        for level, im in enumerate(self.pyr):
            g = geo[level]
            cand = []
            for (x0, y0, cw, ch, offx, offy) in g["cells"]:
                sub = np.ascontiguousarray(im[y0:y0 + ch, x0:x0 + cw])
                k = oo.fast9_16(sub, self.ini_th)
                if len(k) == 0:
                    k = oo.fast9_16(sub, self.min_th)
                k["x"] += f32(offx)
                k["y"] += f32(offy)
                cand.append(k)
            cand = np.concatenate(cand) if cand else np.zeros(0, KP)
            self.cand.append(cand)
            n, idx = oo.distribute_octtree(cand, g["minB"], g["maxBX"], g["minB"], g["maxBY"], self.per[level])
            if n < 0:
                raise UndefinedGeometry("BAD_ASPECT", level, "nIni == 0")
            kps = cand[idx].copy()
            kps["x"] += f32(g["minB"])
            kps["y"] += f32(g["minB"])
            kps["octave"] = level
            kps["size"] = f32(int(f32(PATCH) * self.sf[level]))
            self.kps.append(kps)
        for level, kps in enumerate(self.kps):
            im = self.pyr[level]                       # a strided view is what IC_Angle reads (step = temp's)
            base = im.ctypes.data
            for i in range(len(kps)):
                self.L.orc_ic_angle.restype = C.c_float
                kps["angle"][i] = self.L.orc_ic_angle(C.c_void_p(base), im.strides[0], _round(kps["x"][i]), _round(kps["y"][i]))

    def extract(self, img, cap=None):
        img = np.ascontiguousarray(img, np.uint8)
        self.compute_pyramid(img)
        self.compute_keypoints()
        self.blur = [None] * self.nlevels
        out_k, out_d = [], []
        for level, kps in enumerate(self.kps):
            if not len(kps):
                continue
            work = oo.gaussian_blur7(np.ascontiguousarray(self.pyr[level]))     # GaussianBlur of the level (upstream: of its clone)
            self.blur[level] = work
            d = np.zeros((len(kps), 32), np.uint8)
            for i in range(len(kps)):
                self.L.orc_descriptor(_p(work), work.strides[0], _round(kps["x"][i]), _round(kps["y"][i]),
                                      C.c_float(float(kps["angle"][i])), self.fp_mode, _p(d[i]))
            k = kps.copy()
            if level:
                k["x"] *= self.sf[level]
                k["y"] *= self.sf[level]
            out_k.append(k)
            out_d.append(d)
        k = np.concatenate(out_k) if out_k else np.zeros(0, KP)
        d = np.concatenate(out_d) if out_d else np.zeros((0, 32), np.uint8)
        if cap is not None and len(k) > cap:
            return -4, None, None
        return len(k), k, d

    def level_image(self, level, blur=False):
        a = self.blur[level] if blur else self.pyr[level]
        return None if a is None else np.ascontiguousarray(a)

    def level_candidates(self, level):
        return self.cand[level]

    def level_keypoints(self, level):
        return self.kps[level]


def block_image(seed, w, h, b, levels=256):
    """seeded random grey blocks of b x b pixels: dense corners at every pyramid level"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, levels, ((h + b - 1) // b, (w + b - 1) // b))
    return np.kron(g, np.ones((b, b), np.int64))[:h, :w].astype(np.uint8)

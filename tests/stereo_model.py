"""Frame::ComputeStereoMatches (reference src/Frame.cc:880-1176) as plain numpy, transcribed line by line from the reference text
(the line numbers in the comments), not from oracle/orb_oracle_match.c or the kernels; it never calls the oracle.  Every float step
is one np.float32 operation in the reference's order; the SAD is an exact integer.

Two deviations, the ones the library documents: rows outside [0, nRows) are dropped where the reference indexes vRowIndices
out of bounds (F6, :941 and :968), and a rowRange / colRange outside the level (cv::Mat would assert, :1040-1042, :1079-1083)
means "no match".  An empty vDistIdx (:1161 reads element 0 of it) gives 0 matches.

reason[iL] is the line at which left keypoint iL left the function."""
import math

import numpy as np

f32 = np.float32

ROW_CLAMPED = 1      # F6: (int)vL outside the row table (:968)
NO_CANDIDATE = 2     # vCandidates.empty() (:969)
MAXU_NEG = 3         # maxU < 0 (:977)
ORB_DIST = 4         # bestDist >= thOrbDist (:1022), no gated candidate included
Y0_NEG = 5           # rowRange start < 0 (:1041)
Y1_OVER = 6          # rowRange end > rows (:1041)
X0_NEG = 7           # colRange start < 0 (:1042)
X1_OVER = 8          # colRange end > cols (:1042)
INIU_NEG = 9         # iniu < 0 (:1071)
ENDU_OVER = 10       # endu >= cols (:1072)
BESTINC_END = 11     # bestincR == -L || bestincR == L (:1105)
DELTA_RANGE = 12     # deltaR outside [-1, 1] (:1128)
DISPARITY_RANGE = 13  # !(disparity >= minD && disparity < maxD) (:1135)
CLAMPED = 14         # matched through disparity <= 0 -> 0.01 (:1138-1142), kept by the cut
MATCHED = 15         # matched, kept by the cut
CUT = 16             # matched, then removed by the median cut (:1164-1175)
NAMES = {v: k for k, v in list(globals().items()) if k.isupper() and isinstance(v, int)}

TH_HIGH, TH_LOW = 100, 50   # include/ORBmatcher.h


def c_round(v):
    """::round of a float: half away from zero"""
    v = float(v)
    return f32(math.copysign(math.floor(abs(v) + 0.5), v))


def descriptor_distance(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def stereo_model(kL, dL, kR, dR, scale, inv_scale, pyrL, pyrR, mb, mbf):
    N, Nr = len(kL), len(kR)
    scale = [f32(s) for s in scale]
    inv_scale = [f32(s) for s in inv_scale]
    mb, mbf = f32(mb), f32(mbf)
    uRight = np.full(N, -1.0, f32)                                  # :903-904
    depth = np.full(N, -1.0, f32)
    sad = np.full(N, -1, np.int64)
    reason = np.zeros(N, np.int32)
    thOrbDist = (TH_HIGH + TH_LOW) // 2                             # :907
    nRows = pyrL[0].shape[0]                                        # :910
    vRowIndices = [[] for _ in range(nRows)]                        # :918
    for iR in range(Nr):                                            # :926-942
        kpY = f32(kR["y"][iR])
        r = f32(f32(2.0) * scale[int(kR["octave"][iR])])
        maxr = int(math.ceil(float(f32(kpY + r))))
        minr = int(math.floor(float(f32(kpY - r))))
        for yi in range(minr, maxr + 1):
            if 0 <= yi < nRows:                                     # F6
                vRowIndices[yi].append(iR)
    minZ = mb                                                       # :950-952
    minD = f32(0)
    maxD = f32(mbf / minZ)
    vDistIdx = []
    for iL in range(N):                                             # :959
        levelL = int(kL["octave"][iL])
        vL, uL = f32(kL["y"][iL]), f32(kL["x"][iL])
        row = int(vL)                                               # vRowIndices[vL]: float -> index truncates
        if row < 0 or row >= nRows:
            reason[iL] = ROW_CLAMPED
            continue
        vCandidates = vRowIndices[row]
        if not vCandidates:
            reason[iL] = NO_CANDIDATE
            continue
        minU = f32(uL - maxD)                                       # :973-974
        maxU = f32(uL - minD)
        if maxU < 0:
            reason[iL] = MAXU_NEG
            continue
        bestDist, bestIdxR = TH_HIGH, 0
        for iR in vCandidates:                                      # :990-1018
            octR = int(kR["octave"][iR])
            if octR < levelL - 1 or octR > levelL + 1:
                continue
            uR = f32(kR["x"][iR])
            if uR >= minU and uR <= maxU:
                dist = descriptor_distance(dL[iL], dR[iR])
                if dist < bestDist:
                    bestDist, bestIdxR = dist, iR
        if not bestDist < thOrbDist:                                # :1022
            reason[iL] = ORB_DIST
            continue
        uR0 = f32(kR["x"][bestIdxR])
        scaleFactor = inv_scale[levelL]
        scaleduL = c_round(f32(uL * scaleFactor))                   # :1031-1033
        scaledvL = c_round(f32(vL * scaleFactor))
        scaleduR0 = c_round(f32(uR0 * scaleFactor))
        w = 5
        imL, imR = pyrL[levelL], pyrR[levelL]
        rows, cols = imL.shape
        y0, y1 = int(f32(scaledvL - w)), int(f32(f32(scaledvL + w) + 1))   # :1041
        x0, x1 = int(f32(scaleduL - w)), int(f32(f32(scaleduL + w) + 1))   # :1042
        if y0 < 0:
            reason[iL] = Y0_NEG
            continue
        if y1 > rows:
            reason[iL] = Y1_OVER
            continue
        if x0 < 0:
            reason[iL] = X0_NEG
            continue
        if x1 > cols:
            reason[iL] = X1_OVER
            continue
        IL = imL[y0:y1, x0:x1].astype(np.int64)
        IL = IL - IL[w, w]                                          # :1046
        bestDistS, bestincR = 2147483647, 0                         # :1049-1052
        L = 5
        vDists = [f32(0)] * (2 * L + 1)
        iniu = f32(f32(scaleduR0 - L) - w)                          # :1067-1068
        endu = f32(f32(f32(scaleduR0 + L) + w) + 1)
        if iniu < 0:
            reason[iL] = INIU_NEG
            continue
        if endu >= imR.shape[1]:
            reason[iL] = ENDU_OVER
            continue
        for incR in range(-L, L + 1):                               # :1076-1101
            c0 = int(f32(f32(scaleduR0 + incR) - w))
            c1 = int(f32(f32(f32(scaleduR0 + incR) + w) + 1))
            IR = imR[y0:y1, c0:c1].astype(np.int64)
            IR = IR - IR[w, w]
            s = 0
            for v in np.abs(IL - IR).ravel().tolist():              # cv::norm(NORM_L1): integer-valued, exact
                s += v
            dist = f32(s)
            if dist < f32(bestDistS):
                bestDistS, bestincR = int(dist), incR
            vDists[L + incR] = dist
        if bestincR == -L or bestincR == L:                         # :1105
            reason[iL] = BESTINC_END
            continue
        dist1, dist2, dist3 = vDists[L + bestincR - 1], vDists[L + bestincR], vDists[L + bestincR + 1]
        with np.errstate(all="ignore"):
            den = f32(f32(2.0) * f32(f32(dist1 + dist3) - f32(f32(2.0) * dist2)))
            deltaR = f32(f32(dist1 - dist3) / den)                  # :1125
        if deltaR < -1 or deltaR > 1:
            reason[iL] = DELTA_RANGE
            continue
        bestuR = f32(scale[levelL] * f32(f32(scaleduR0 + f32(bestincR)) + deltaR))   # :1132
        disparity = f32(uL - bestuR)
        if disparity >= minD and disparity < maxD:                  # :1135
            reason[iL] = MATCHED
            if disparity <= 0:
                disparity = f32(0.01)                               # double constants stored to float (:1140-1141)
                bestuR = f32(float(uL) - 0.01)
                reason[iL] = CLAMPED
            depth[iL] = f32(mbf / disparity)
            uRight[iL] = bestuR
            sad[iL] = bestDistS
            vDistIdx.append((bestDistS, iL))
        else:
            reason[iL] = DISPARITY_RANGE
    n = len(vDistIdx)
    if vDistIdx:                                                    # :1160-1175
        vDistIdx.sort()
        median = f32(vDistIdx[len(vDistIdx) // 2][0])
        thDist = f32(f32(f32(1.5) * f32(1.4)) * median)
        for i in range(len(vDistIdx) - 1, -1, -1):
            if f32(vDistIdx[i][0]) < thDist:
                break
            uRight[vDistIdx[i][1]] = -1
            depth[vDistIdx[i][1]] = -1
            reason[vDistIdx[i][1]] = CUT
            n -= 1
    return n, uRight, depth, sad, reason

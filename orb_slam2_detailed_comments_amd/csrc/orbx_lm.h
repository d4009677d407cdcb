// orbx_lm.h -- what g2o executes around ONE free vertex with a dense N x N system, stated once for the optimizers of the library
// (Optimizer::PoseOptimization: orbx_pose.h, N = 6; Optimizer::OptimizeSim3: orbx_sim3opt.h, N = 7): RobustKernelHuber, the
// unpivoted L D L^T solve and OptimizationAlgorithmLevenberg::solve inside SparseOptimizer::optimize (orbx_pose_rounds keeps that
// loop written out in place, see there).  tests/lm_model.py restates it independently in numpy float64.  The bottom of the
// header family: header-only, HIP-free in a host unit, no other header of the library is included.
//
// fp_mode: every expression is written operation by operation and the library is built with -ffp-contract=off, so nothing here
// is contracted; division and square root are the correctly rounded IEEE double operations on the host and on the device.
#pragma once
#include <math.h>
#include <stdint.h>
#include "../../include/orbx.h"
#if defined(__HIPCC__)
#ifndef ORBX_HD
#define ORBX_HD __host__ __device__
#endif
#else
#ifndef ORBX_HD
#define ORBX_HD
#endif
#endif

#if defined(__clang__)
#define ORBX_UNROLL _Pragma("unroll")
#else
#define ORBX_UNROLL
#endif

#define ORBX_DBL_MAX 0x1.fffffffffffffp+1023
enum { ORBX_LM_TRIALS = 10 };                                  // _maxTrialsAfterFailure
// One edge's terms, and their sums over the edges, in this order: the upper triangle of H row by row, b, rho0
template <int N> struct OrbxLm { enum { B = N * (N + 1) / 2, CHI = B + N, TERMS = CHI + 1 }; };

ORBX_HD static inline bool orbx_finite(double v) { return __builtin_fabs(v) <= ORBX_DBL_MAX; }

// RobustKernelHuber::robustify: returns rho0, *rho1 = rho'
ORBX_HD static inline double orbx_lm_huber(double chi2, double delta, double *rho1) {
    *rho1 = 1.0;
    const double dsqr = delta * delta;
    if (chi2 <= dsqr) return chi2;
    const double sq = sqrt(chi2);
    *rho1 = delta / sq;
    return 2.0 * sq * delta - dsqr;
}
// acc = acc (+) t for one edge, in the order every caller adds edges: H and chi by addition, b by subtraction (b -= ...)
template <int N> ORBX_HD static inline double orbx_lm_accumulate(int term, double acc, double t) {
    return term >= OrbxLm<N>::B && term < OrbxLm<N>::CHI ? acc - t : acc + t;
}

// (H + lambda I) x = b by an unpivoted L D L^T (H: upper triangle row by row).  The system counts as positive, and is solved,
// when every pivot d_j is > 0 and finite; otherwise the solve fails and x = 0.
template <int N> ORBX_HD static inline bool orbx_lm_solve(const double *H, double lambda, const double *b, double *x) {
    double A[N * N], L[N * N], d[N], w[N], y[N];
    {
        int n = 0;
ORBX_UNROLL
        for (int j = 0; j < N; ++j)
ORBX_UNROLL
            for (int k = j; k < N; ++k) { const double v = j == k ? H[n] + lambda : H[n]; A[N * j + k] = v; A[N * k + j] = v; ++n; }
    }
    bool ok = true;
ORBX_UNROLL
    for (int j = 0; j < N; ++j) {
        double s = A[N * j + j];
ORBX_UNROLL
        for (int k = 0; k < j; ++k) { w[k] = L[N * j + k] * d[k]; s = s - L[N * j + k] * w[k]; }
        d[j] = s;
        if (!(s > 0 && s <= ORBX_DBL_MAX)) ok = false;
ORBX_UNROLL
        for (int i = j + 1; i < N; ++i) {
            double t = A[N * i + j];
ORBX_UNROLL
            for (int k = 0; k < j; ++k) t = t - L[N * i + k] * w[k];
            L[N * i + j] = t / s;
        }
    }
    if (!ok) {
ORBX_UNROLL
        for (int i = 0; i < N; ++i) x[i] = 0.0;
        return false;
    }
ORBX_UNROLL
    for (int i = 0; i < N; ++i) {
        double s = b[i];
ORBX_UNROLL
        for (int k = 0; k < i; ++k) s = s - L[N * i + k] * y[k];
        y[i] = s;
    }
ORBX_UNROLL
    for (int i = N - 1; i >= 0; --i) {
        double s = y[i] / d[i];
ORBX_UNROLL
        for (int k = i + 1; k < N; ++k) s = s - L[N * k + i] * x[k];
        x[i] = s;
    }
    return true;
}

// SparseOptimizer::optimize(iters) with OptimizationAlgorithmLevenberg::solve: lambda and nu start anew at iteration 0
// (computeLambdaInit), at most ten trials per iteration, Terminate, the "Raul" stop, chi' = DBL_MAX on a failed solve.  est carries
// over; last = where computeActiveErrors ran last (a rejected last trial included).  Step supplies the passes over the edges and
// the vertex; everything here is uniform over the lanes of a wave that run it side by side:
//   void system(est, acc[TERMS])     computeActiveErrors + activeRobustChi2 + buildSystem at est, edge order
//   double chi(est)                  computeActiveErrors + activeRobustChi2 at est
//   Est oplus(est, x[N])             oplusImpl; may write x (computeScale reads it afterwards)
template <int N, class Step, class Est> ORBX_HD static inline void orbx_lm_optimize(Step &step, int iters, Est &est, Est &last) {
    typedef OrbxLm<N> T;
    double lambda = 0.0, nu = 2.0;
    int stall = 0;
    for (int it = 0; it < iters; ++it) {
        double acc[T::TERMS], x[N];
        step.system(est, acc);
        last = est;
        double cur = acc[T::CHI];
        const double ini = cur;
        if (it == 0) {                                         // computeLambdaInit: tau * max |H_jj|, std::max as written
            double m = 0.0;
            int dg = 0;                                        // H_jj sits N - j terms after H_(j-1)(j-1)
ORBX_UNROLL
            for (int j = 0; j < N; ++j) { const double a = __builtin_fabs(acc[dg]); m = a < m ? m : a; dg += N - j; }
            lambda = 1e-5 * m;
            nu = 2.0;
            stall = 0;
        }
        double rho = 0.0;
        int q = 0;
        do {
            const Est backup = est;
            const bool ok = orbx_lm_solve<N>(acc, lambda, acc + T::B, x);
            est = step.oplus(est, x);
            double tmp = step.chi(est);
            last = est;
            if (!ok) tmp = ORBX_DBL_MAX;
            rho = cur - tmp;
            double scale = 0.0;
ORBX_UNROLL
            for (int j = 0; j < N; ++j) scale = scale + x[j] * (lambda * x[j] + acc[T::B + j]);
            scale = scale + 1e-3;
            rho = rho / scale;
            if (rho > 0 && orbx_finite(tmp)) {
                const double r2 = 2.0 * rho - 1.0;
                double alpha = 1.0 - (r2 * r2) * r2;
                alpha = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;
                const double sf = (1.0 / 3.0) < alpha ? alpha : (1.0 / 3.0);
                lambda = lambda * sf;
                nu = 2.0;
                cur = tmp;
            } else {
                lambda = lambda * nu;
                nu = nu * 2.0;
                est = backup;
            }
            ++q;
        } while (rho < 0 && q < ORBX_LM_TRIALS);
        if (q == ORBX_LM_TRIALS || rho == 0) break;            // Terminate
        if ((ini - cur) * 1e3 < ini) ++stall; else stall = 0;
        if (stall >= 3) break;                                  // Stop criterium (Raul)
    }
}

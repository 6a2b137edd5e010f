// gfx950 kernels for a smoothed constant-velocity track (KF_MODEL_CV2 / KF_MODEL_CV3 with a
// block-diagonal P and a diagonal R): cv_rec_kernel, kf_run's fused run that also records the
// filtered covariance (kf_run_rec), and cv_smooth_kernel, the Rauch-Tung-Striebel backward pass
// over that record (kf_smooth_run).  Template flags of the same two kernels give every filter its
// own q_pos, q_vel and R and score the run where it runs (kf_run_scores), and smooth under the same
// per-filter Q (kf_smooth_run_params); one more on the smoother adds the EM statistics for Q and R
// and the smoothed row before step 0 (kf_smooth_run_em).
//
// Mapping, as in kf_cv.hip: ONE FILTER PER LANE, kBlock lanes per workgroup.  P is block-diagonal
// over the axes, so a filter is D independent 2-state (pos_i, vel_i) chains: per axis x = (p, v)
// and P_i = (pp, pv, vv) live in VGPRs, and every record row is one coalesced [B]-long SoA row
// addressed from a 64-bit base (row_rsrc) plus the lane's 32-bit offset.  Both kernels are bound
// by HBM bytes at bench sizes; the inputs come through a fully unrolled register ring so the
// loads of later steps are in flight while a step computes.  No LDS, no atomics, no workspace.
#include <hip/hip_runtime.h>
#include <math.h>

#include <stdint.h>

#include <type_traits>

#include "kf_common.h"
#include "kf_internal.h"

namespace kfmi {
namespace {

using namespace dev;

// Inputs of one forward step (kf_cv.hip's StepIn).
template <int D, typename T>
struct RecIn {
    T u[D];
    T z[D];
    uint8_t use;
};
// SCORED: the step's track row rides in the ring with its other inputs
template <int D, typename T>
struct RecInScored : RecIn<D, T> {
    T tr[D];
};

// SCORED: a lane's score accumulators (kf_run_scores).  Doubles whatever the handle's dtype; the
// product of every applied S is a running (mantissa, binary exponent) pair, logged once at the end
// (kf_ref_chainlane.h's ScoreAcc, one filter per lane)
struct CvScoreAcc {
    int32_t ngps = 0;   // applied fixes
    double nis = 0.0;   // sum over them of sum_axis y^2 / S
    double ldm = 1.0;   // product of their S: mantissa ...
    int32_t lde = 0;    // ... and binary exponent
    int32_t npos = 0;   // steps scored against the track
    double sse = 0.0;   // sum over them of sum_axis (pos - track)^2
};
struct NoCvScore {};

__device__ __forceinline__ const CvRecArgs& rec_args(const CvRecArgs& a) { return a; }
__device__ __forceinline__ const CvRecArgs& rec_args(const CvScoreArgs& a) { return a.rec; }

// ------------------------------------------------------------------------------------
// kf_run_rec: cv_block_kernel (kf_cv.hip) with the filtered covariance recorded after every
// step, cov [T][3 D][B], rows 3 i .. 3 i + 2 = axis i's (pp, pv, vv).
//   THE PREDICT, UPDATE, POISON AND LOG-DET LINES BELOW ARE cv_block_kernel's, REPEATED IN ITS
//   ORDER.  A change to either copy must be made to both (tests/test_gpu_cv_smoother.py compares
//   the two with ==).
// GENERAL = false is cv_block_kernel's input shape (scalar dt, u, no mask).  GENERAL = true: what
// cv_block_kernel leaves to cv_run_kernel<GENERAL> is decided by wave-uniform branches and
// zero-length row descriptors, as there: dt_steps (dt, dt^2 / 2 and Q dt per step, from the same
// expressions), a NULL u (loads return 0) and a mask (a masked lane keeps its prediction).
// REC_OPT: traj, cov and logdet may each be NULL (stores dropped by the range check; a NULL logdet
// is not computed and then does not reach the status either, as in cv_run_kernel).
// State, status, traj and logdet are bit for bit those of the kf_run call with the same inputs
// and both of its records, on either of its kernels (the block and the general kernel agree on a
// block-diagonal P).  Which records are NULL never changes a bit here.  It does in kf_run, in
// fp64: with a record missing it runs cv_run_kernel<GENERAL = true>, whose Q dt is formed in the
// step and contracted into the sum it enters, one rounding fewer than the hoisted Q dt of the
// fast shape (see `step` below).
// PARAMS / SCORED (kf_run_scores; the argument block is then CvScoreArgs, A): everything they add
// sits under `if constexpr`, and the instantiations without them are instruction for instruction
// what they were (profiles/cv_scores/isa_compare.log).
// PARAMS: q_pos, q_vel and the diagonal of R are the lane's column of ka.consts, loaded once before
// the first step (a NULL table: the handle's, by a wave-uniform select); each enters the
// expressions the handle's own constant enters, T(q * dt) formed in double where each shape forms
// it, so either shape keeps its own rounding of Q dt + P and column f is kf_run_rec on a handle
// holding column f's values, bit for bit.
// SCORED: lane-local accumulators, no atomics and no reduction.  The update's own y, S and 1 / S
// give the NIS and the running product of S (a masked lane adds 0 and multiplies by 1); the track
// row of step t comes through the ring and is scored after the step unless one of its D values is
// NaN.  A NULL track or a NULL scores table costs nothing but the arithmetic: zero-length rows.
// ------------------------------------------------------------------------------------
template <int D, typename T, int DEPTH, bool GENERAL, bool REC_OPT, bool PARAMS = false, bool SCORED = false,
          typename A = CvRecArgs>
__global__ __launch_bounds__(kBlock) void cv_rec_kernel(const A ka) {
    static_assert(std::is_same_v<A, std::conditional_t<PARAMS || SCORED, CvScoreArgs, CvRecArgs>>, "argument block");
    constexpr int N = 2 * D;
    const CvRecArgs& ra = rec_args(ka);
    const CvArgs& a = ra.run;
    const int64_t f = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (f >= a.B) return;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(a.B) * uint32_t(sizeof(T));
    const bool has_dts = GENERAL && a.dt_steps != nullptr;
    const bool has_mask = GENERAL && a.mask != nullptr;
    const bool has_ld = !REC_OPT || a.logdet != nullptr;
    T xp[D], xv[D], pp[D], pv[D], vv[D], r[D];
#pragma unroll
    for (int i = 0; i < D; ++i) {
        xp[i] = ldb<T>(a.x, i, rb, off);
        xv[i] = ldb<T>(a.x, D + i, rb, off);
        pp[i] = ldb<T>(a.P, tri<N>(i, i), rb, off);
        pv[i] = ldb<T>(a.P, tri<N>(i, D + i), rb, off);
        vv[i] = ldb<T>(a.P, tri<N>(D + i, D + i), rb, off);
        r[i] = T(a.r[tri<D>(i, i)]);
    }
    double q_lane[2] = {0.0, 0.0};  // PARAMS: the lane's q_pos, q_vel
    if constexpr (PARAMS) {
        q_lane[0] = a.q_pos;
        q_lane[1] = a.q_vel;
        if (ka.consts != nullptr) {  // wave-uniform
            const uint32_t off8 = uint32_t(f) * 8u, rb8 = uint32_t(a.B) * 8u;
            q_lane[0] = ldb<double>(ka.consts, 0, rb8, off8);
            q_lane[1] = ldb<double>(ka.consts, 1, rb8, off8);
#pragma unroll
            for (int i = 0; i < D; ++i) r[i] = T(ldb<double>(ka.consts, 2 + i, rb8, off8));
        }
    }
    int32_t st = a.status[f];
    const int T_ = a.T;
    const int k_upd = a.update_every;
    const int U = T_ / k_upd;
    int ld_upd_step = k_upd - 1;
    int ld_s = 0;
    const uint32_t rb_u = (!GENERAL || a.u != nullptr) ? rb : 0u;
    const uint32_t rb_z = U > 0 ? rb : 0u;
    const uint32_t rb_tr = (!REC_OPT || a.traj != nullptr) ? rb : 0u;  // absent records: stores dropped
    const uint32_t rb_cov = (!REC_OPT || ra.cov != nullptr) ? rb : 0u;
    const uint32_t rb_m = (has_mask && U > 0) ? uint32_t(a.B) : 0u;  // mask rows are [B] bytes
    const T dt0 = T(a.dt);
    const T hdt20 = T(0.5) * dt0 * dt0;
    // (the handle's constants stay read from the argument block in their own expressions: routing
    // them through a local changed the existing instantiations' instruction streams)
    T qp0, qv0;
    if constexpr (PARAMS) {
        qp0 = T(q_lane[0] * a.dt);
        qv0 = T(q_lane[1] * a.dt);
    } else {
        qp0 = T(a.q_pos * a.dt);
        qv0 = T(a.q_vel * a.dt);
    }
    using In = std::conditional_t<SCORED, RecInScored<D, T>, RecIn<D, T>>;
    std::conditional_t<SCORED, CvScoreAcc, NoCvScore> sc;
    bool has_track = false;
    uint32_t rb_tk = 0u;
    if constexpr (SCORED) {
        has_track = ka.track != nullptr;
        rb_tk = has_track ? rb : 0u;
    }
    auto load_in = [&](int t, In& in) {
        const int tc = t < T_ ? t : T_ - 1;
        if (tc > ld_upd_step) {
            ld_upd_step += k_upd;
            ++ld_s;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) in.u[i] = ldb_stream(a.u, int64_t(tc) * D + i, rb_u, off, T(0));
        int s = ld_s < U ? ld_s : U - 1;
        s = s > 0 ? s : 0;
        const bool upd = tc == ld_upd_step;  // wave-uniform
        const uint32_t rbz = upd ? rb_z : 0u;  // z only on update steps
#pragma unroll
        for (int i = 0; i < D; ++i) in.z[i] = ldb_stream(a.z, int64_t(s) * D + i, rbz, off, T(0));
        // a zero-length row (no mask, or no update at this step) loads 0: no branch, no address
        in.use = GENERAL ? ldb<uint8_t>(a.mask, s, upd ? rb_m : 0u, uint32_t(f)) : uint8_t(1);
        if constexpr (SCORED) {
#pragma unroll
            for (int i = 0; i < D; ++i) in.tr[i] = ldb_stream(ka.track, int64_t(tc) * D + i, rb_tk, off, T(0));
        }
    };
    int until_upd = k_upd;
    auto step = [&](int t, const In& in) {
        // GENERAL: cv_run_kernel's per-step dt in its own expressions, statement for statement.  The
        // shape matters, not only the values: with Q dt formed in the step, next to the sum it
        // enters, the compiler contracts q dt + P into one fma in fp64 there and here alike
        // (-ffp-contract=fast), and with Q dt hoisted (cv_block_kernel, GENERAL = false) it does
        // not; kf_run's two routes differ by that rounding, and each instantiation follows its own
        T dt = dt0, hdt2 = hdt20, qp = qp0, qv = qv0;
        if constexpr (GENERAL) {
            const double dtd = has_dts ? a.dt_steps[t] : a.dt;
            dt = T(dtd);
            hdt2 = T(0.5) * dt * dt;
            if constexpr (PARAMS) {
                qp = T(q_lane[0] * dtd);
                qv = T(q_lane[1] * dtd);
            } else {
                qp = T(a.q_pos * dtd);
                qv = T(a.q_vel * dtd);
            }
        }
        // predict (Cv::predict per axis): Bm' = Bm + dt C, A' = A + dt (Bm' + Bm^T), + Q
#pragma unroll
        for (int i = 0; i < D; ++i) {
            xp[i] = fmaT(hdt2, in.u[i], fmaT(dt, xv[i], xp[i]));
            xv[i] = fmaT(dt, in.u[i], xv[i]);
            const T bn = fmaT(dt, vv[i], pv[i]);
            pp[i] = fmaT(dt, bn + pv[i], pp[i]);
            pv[i] = bn;
            pp[i] += qp;
            vv[i] += qv;
        }
        if (--until_upd == 0) {  // wave-uniform
            until_upd = k_upd;
            // the mask is per lane: a masked lane computes the update and keeps its old values
            // (selects, no divergent branch)
            const bool app = !has_mask || in.use;
            bool ok = true;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                // sel_update with a diagonal S: one scalar pivot per axis, Joseph form
                const T S = pp[i] + r[i];
                ok = ok && (S > T(0));
                const T dinv = rcp_pos<2>(S);
                const T k0 = pp[i] * dinv, k1 = pv[i] * dinv;
                const T y = in.z[i] - xp[i];
                if constexpr (SCORED) {
                    // the update's own y, S and reciprocal; a masked lane adds 0 and multiplies by 1
                    const T term = (y * y) * dinv;
                    sc.nis += app ? double(term) : 0.0;
                    sc.ldm *= app ? double(S) : 1.0;
                }
                const T nxp = fmaT(k0, y, xp[i]);
                const T nxv = fmaT(k1, y, xv[i]);
                const T e0 = fmaT(k0, S, -pp[i]);
                const T e1 = fmaT(k1, S, -pv[i]);
                const T npp = fmaT(e0, k0, fmaT(-k0, pp[i], pp[i]));
                const T npv = fmaT(e0, k1, fmaT(-k0, pv[i], pv[i]));
                const T nvv = fmaT(e1, k1, fmaT(-k1, pv[i], vv[i]));
                // a bad pivot poisons the whole filter, as in the general kernel
                xp[i] = app ? nxp : xp[i];
                xv[i] = app ? nxv : xv[i];
                pp[i] = app ? npp : pp[i];
                pv[i] = app ? npv : pv[i];
                vv[i] = app ? nvv : vv[i];
            }
            const T poison = ok ? T(0) : quiet_nan<T>();
#pragma unroll
            for (int i = 0; i < D; ++i) {
                xp[i] = app ? xp[i] + poison : xp[i];
                xv[i] = app ? xv[i] + poison : xv[i];
                pp[i] = app ? pp[i] + poison : pp[i];
                pv[i] = app ? pv[i] + poison : pv[i];
                vv[i] = app ? vv[i] + poison : vv[i];
            }
            st = (ok || !app) ? st : kNotSpd;
            if constexpr (SCORED) {
                renorm(sc.ldm, sc.lde);
                sc.ngps += app ? 1 : 0;
            }
        }
        if constexpr (SCORED) {
            // the position after the step against the track row, both as doubles
            bool have = has_track;
            double e2 = 0.0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                have = have && (in.tr[i] == in.tr[i]);
                const double e = double(xp[i]) - double(in.tr[i]);
                e2 = fmaT(e, e, e2);
            }
            sc.sse += have ? e2 : 0.0;
            sc.npos += have ? 1 : 0;
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            stb_rec(a.traj, int64_t(t) * N + i, rb_tr, off, xp[i]);
            stb_rec(a.traj, int64_t(t) * N + D + i, rb_tr, off, xv[i]);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            stb_rec(ra.cov, int64_t(t) * (3 * D) + 3 * i, rb_cov, off, pp[i]);
            stb_rec(ra.cov, int64_t(t) * (3 * D) + 3 * i + 1, rb_cov, off, pv[i]);
            stb_rec(ra.cov, int64_t(t) * (3 * D) + 3 * i + 2, rb_cov, off, vv[i]);
        }
        if (has_ld) {  // wave-uniform
            // logdet: LDL pivots in the general 6x6 order (positions, then velocities)
            T prod = T(1);
            int ex = 0, e;
            bool pd = true;
            T dv[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                pd = pd && (pp[i] > T(0));
                prod *= pp[i];
                const T l = pv[i] * rcp_nr<1>(pp[i]);
                const T v = l * pp[i];
                dv[i] = fmaT(-l, v, vv[i]);
            }
            prod = frexp(prod, &e);
            ex += e;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                pd = pd && (dv[i] > T(0));
                prod *= dv[i];
            }
            prod = frexp(prod, &e);
            ex += e;
            const T ld = pd ? log_mant(prod, ex) : quiet_nan<T>();
            st = (ld == ld) ? st : kNotSpd;
            stb_rec(a.logdet, t, rb, off, ld);
        }
    };
    // cv_block_kernel's input ring: DEPTH statically named buffers, prologue drained once
    In buf[DEPTH];
#pragma unroll
    for (int j = 0; j < DEPTH - 1; ++j) load_in(j, buf[j]);
    __builtin_amdgcn_s_waitcnt(0);
    int t = 0;
    for (; t + DEPTH <= T_; t += DEPTH) {
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            load_in(t + j + DEPTH - 1, buf[(j + DEPTH - 1) % DEPTH]);
            step(t + j, buf[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < DEPTH - 1; ++j)
        if (t + j < T_) step(t + j, buf[j]);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        stb(a.x, i, rb, off, xp[i]);
        stb(a.x, D + i, rb, off, xv[i]);
        stb(a.P, tri<N>(i, i), rb, off, pp[i]);
        stb(a.P, tri<N>(i, D + i), rb, off, pv[i]);
        stb(a.P, tri<N>(D + i, D + i), rb, off, vv[i]);
    }
    a.status[f] = st;
    if constexpr (SCORED) {
        // rows KF_SCORE_*: the IMU rows are 0; a filter that is not KF_OK keeps its counts only
        const uint32_t off8 = uint32_t(f) * 8u;
        const uint32_t rb8 = ka.scores != nullptr ? uint32_t(a.B) * 8u : 0u;
        const bool good = st == 0;
        const double nanv = quiet_nan<double>();
        stb(ka.scores, kScoreGpsN, rb8, off8, double(sc.ngps));
        stb(ka.scores, kScoreGpsNis, rb8, off8, good ? sc.nis : nanv);
        stb(ka.scores, kScoreGpsLogdetS, rb8, off8, good ? log_mant(sc.ldm, sc.lde) : nanv);
        stb(ka.scores, kScoreImuN, rb8, off8, 0.0);
        stb(ka.scores, kScoreImuNis, rb8, off8, 0.0);
        stb(ka.scores, kScoreImuLogdetS, rb8, off8, 0.0);
        stb(ka.scores, kScorePosN, rb8, off8, double(sc.npos));
        stb(ka.scores, kScorePosSse, rb8, off8, good ? sc.sse : nanv);
    }
}

// ------------------------------------------------------------------------------------
// kf_smooth_run: the RTS backward pass over filt_x [T][2 D][B] / filt_P [T][3 D][B] (kf_run_rec's
// traj and cov), f64.  Row T - 1 is the filtered row.  For t = T - 2 .. 0, per axis, with
// (x_f, P_f) = row t, d = dt[t + 1]:
//   x_p = F x_f + G u[t + 1], P_p = F P_f F^T + Q d   (cv_rec_kernel's predict lines on row t: the
//                                                     forward run's P_pred, up to the one rounding
//                                                     of Q d + P that its two input shapes differ by)
//   C = (P_f F^T) P_p^-1                              (2 x 2 LDL^T of P_p in-lane; its two pivots'
//                                                     reciprocals are IEEE divisions, as in
//                                                     ref_smooth_kernel: P_f - C P_p C^T cancels)
//   x_s[t] = x_f + C (x_s[t + 1] - x_p)
//   P_s[t] = P_f + C (P_s[t + 1] - P_p) C^T           (once per packed entry)
// The lane carries the smoothed row t + 1, 5 values per axis.  The inputs of row t (2 D states,
// 3 D covariance entries, D controls) come backwards through a ring of DEPTH statically named
// buffers: backward step s is row t = T - 2 - s, loaded DEPTH - 1 steps before step s runs and so
// before the only store that can overwrite it (the lane's own store of row t in step s), which
// makes sm_x == filt_x / sm_P == filt_P equal to running out of place.
// A NaN in a loaded row (state, covariance or control) or a non-positive pivot of P_p poisons the
// filter from that t down to 0: NaN rows, KF_ENOTSPD in sm_status; the rows above are stored.
// sm_logdet takes the LDL pivots of P_s in the forward log-det's order and form.
// PARAMS (kf_smooth_run_params; the argument block is then CvSmoothParamArgs, A): q_pos and q_vel
// are the lane's column of ka.consts (rows 0 and 1 of kf_run_scores' table), loaded once, and enter
// the expressions the handle's own enter; a NULL table selects the handle's.  Without PARAMS the
// kernel is instruction for instruction what it was.
// EM (kf_smooth_run_em; PARAMS too, the argument block is then CvSmoothEmArgs): everything it adds
// sits under `if constexpr`, and the instantiations without it are instruction for instruction
// what they were (profiles/cv_em/isa_compare.log).  Three additions, all lane-local, summed in
// double in backward step order, no atomics and no reduction:
//   the row before step 0: with init_x / init_P one more backward step takes them as the filtered
//   row before step 0 (d = dt[0], u[0]) and stores its smoothed row to sm_init_x / sm_init_P;
//   the noise sums: the transition into step t + 1 has w = x[t + 1] - F x[t] - G u[t + 1], and with
//   J = Q d P_p^-1 (the step's own LDL^T of P_p) E[w | all] = J (x_s[t + 1] - x_p) and
//   Var[w | all] = Q d + J (P_s[t + 1] - P_p) J^T: the differences the smoothing step has already
//   formed, nothing of P_s[t]; the two diagonal entries of E[w] E[w]^T + Var over d are added per
//   axis, axes in order; a transition with d == 0 adds nothing and is not counted (wave-uniform);
//   the R sums: the fix z[t / k] of a step the forward run updated at rides in the ring (zero-length
//   rows elsewhere, as in cv_rec_kernel) with its mask byte, and after row t is smoothed axis i adds
//   (z_i - p_s,i)^2 + P_s[pp]_i.
// A filter whose status is not 0 has NaN in its float rows; its counts still count.
// ------------------------------------------------------------------------------------
#ifndef KF_CV_SMOOTH_DEPTH
#define KF_CV_SMOOTH_DEPTH 4
#endif
constexpr int kCvSmoothDepth = KF_CV_SMOOTH_DEPTH;  // input ring of cv_smooth_kernel

template <int D>
struct SmoothRow {
    double x[2 * D];
    double P[3 * D];
    double u[D];
};
// EM: the step's fix rides in the ring with its other inputs
template <int D>
struct SmoothRowEm : SmoothRow<D> {
    double z[D];
    uint8_t use;
};

// EM: a lane's accumulators (kf_smooth_run_em)
template <int D>
struct CvEmAcc {
    double qp = 0.0;    // sum over the counted transitions of sum_axis E[w_pos^2 | all] / d
    double qv = 0.0;    // ... E[w_vel^2 | all] / d
    double r[D] = {};   // per axis: sum over the applied fixes of (z - p_s)^2 + P_s[pp]
    int32_t nfix = 0;   // applied fixes
    int ntrans = 0;     // transitions counted (wave-uniform)
};
struct NoCvEm {};

__device__ __forceinline__ const CvSmoothArgs& smooth_args(const CvSmoothArgs& a) { return a; }
__device__ __forceinline__ const CvSmoothArgs& smooth_args(const CvSmoothParamArgs& a) { return a.smooth; }
__device__ __forceinline__ const CvSmoothArgs& smooth_args(const CvSmoothEmArgs& a) { return a.p.smooth; }
__device__ __forceinline__ const double* smooth_consts(const CvSmoothParamArgs& a) { return a.consts; }
__device__ __forceinline__ const double* smooth_consts(const CvSmoothEmArgs& a) { return a.p.consts; }

template <int D, int DEPTH, bool PARAMS = false, typename A = CvSmoothArgs, bool EM = false>
__global__ __launch_bounds__(kBlock) void cv_smooth_kernel(const A ka) {
    static_assert(std::is_same_v<A, std::conditional_t<EM, CvSmoothEmArgs,
                                                       std::conditional_t<PARAMS, CvSmoothParamArgs, CvSmoothArgs>>>,
                  "argument block");
    static_assert(PARAMS || !EM, "EM reads the constants' table as PARAMS does");
    using T = double;
    constexpr int N = 2 * D, NP = 3 * D;
    const CvSmoothArgs& a = smooth_args(ka);
    const int64_t f = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (f >= a.B) return;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(a.B) * uint32_t(sizeof(T));
    double q_pos = a.q_pos, q_vel = a.q_vel;
    if constexpr (PARAMS) {
        if (smooth_consts(ka) != nullptr) {  // wave-uniform
            q_pos = ldb<double>(smooth_consts(ka), 0, rb, off);
            q_vel = ldb<double>(smooth_consts(ka), 1, rb, off);
        }
    }
    const bool has_dts = a.dt_steps != nullptr;
    const bool need_ld = a.sm_logdet != nullptr;
    const uint32_t rb_u = a.u != nullptr ? rb : 0u;      // no control: loads return 0
    const uint32_t rb_sx = a.sm_x != nullptr ? rb : 0u;  // absent outputs: stores dropped
    const uint32_t rb_sP = a.sm_P != nullptr ? rb : 0u;
    const int T_ = a.T;

    T sp[D], sv[D], spp[D], spv[D], svv[D];  // the smoothed row t + 1
    int32_t st = 0;
    auto poison = [&]() {
        st = kNotSpd;
#pragma unroll
        for (int i = 0; i < D; ++i) sp[i] = sv[i] = spp[i] = spv[i] = svv[i] = quiet_nan<T>();
    };
    auto store_row = [&](int t) {
#pragma unroll
        for (int i = 0; i < D; ++i) {
            stb_rec(a.sm_x, int64_t(t) * N + i, rb_sx, off, sp[i]);
            stb_rec(a.sm_x, int64_t(t) * N + D + i, rb_sx, off, sv[i]);
        }
#pragma unroll
        for (int i = 0; i < D; ++i) {
            stb_rec(a.sm_P, int64_t(t) * NP + 3 * i, rb_sP, off, spp[i]);
            stb_rec(a.sm_P, int64_t(t) * NP + 3 * i + 1, rb_sP, off, spv[i]);
            stb_rec(a.sm_P, int64_t(t) * NP + 3 * i + 2, rb_sP, off, svv[i]);
        }
        if (need_ld) {  // wave-uniform
            // cv_rec_kernel's log-det lines on P_s: positions, renormalise, velocities, renormalise
            T prod = T(1);
            int ex = 0, e;
            bool pd = true;
            T dv[D];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                pd = pd && (spp[i] > T(0));
                prod *= spp[i];
                const T l = spv[i] * rcp_nr<1>(spp[i]);
                const T v = l * spp[i];
                dv[i] = fmaT(-l, v, svv[i]);
            }
            prod = frexp(prod, &e);
            ex += e;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                pd = pd && (dv[i] > T(0));
                prod *= dv[i];
            }
            prod = frexp(prod, &e);
            ex += e;
            const T ld = pd ? log_mant(prod, ex) : quiet_nan<T>();
            stb_rec(a.sm_logdet, t, rb, off, ld);
        }
    };
    auto load_xP = [&](int t, T (&x)[N], T (&P)[NP]) {
#pragma unroll
        for (int i = 0; i < N; ++i) x[i] = ldb_stream(a.filt_x, int64_t(t) * N + i, rb, off, T(0));
#pragma unroll
        for (int k = 0; k < NP; ++k) P[k] = ldb_stream(a.filt_P, int64_t(t) * NP + k, rb, off, T(0));
    };

    // EM: the accumulators, and the fixes' rows counted down with the loads (rows are loaded in
    // the order T - 1, T - 2, ...: ld_upd is the next update step at or below the row to load)
    std::conditional_t<EM, CvEmAcc<D>, NoCvEm> em;
    bool has_init = false, has_z = false, has_mask = false;
    int k_upd = 1, ld_upd = -1, ld_zi = 0;
    if constexpr (EM) {
        has_init = ka.init_x != nullptr;
        has_z = ka.z != nullptr;
        has_mask = has_z && ka.mask != nullptr;
        k_upd = ka.update_every;
        ld_zi = T_ / k_upd - 1;
        ld_upd = (ld_zi + 1) * k_upd - 1;
    }
    // the fix of row t and whether the lane applied it; live = false: a load past the last step
    auto load_z = [&](int t, bool live, T (&z)[D], uint8_t& use) {
        if constexpr (EM) {
            const bool at = live && t >= 0 && t == ld_upd;  // wave-uniform
            const bool upd = at && has_z;
            const int zi = ld_zi > 0 ? ld_zi : 0;
            const uint32_t rbz = upd ? rb : 0u;  // z only on update steps
#pragma unroll
            for (int i = 0; i < D; ++i) z[i] = ldb_stream(ka.z, int64_t(zi) * D + i, rbz, off, T(0));
            // a zero-length row (no update at this row) loads 0
            use = has_mask ? ldb<uint8_t>(ka.mask, zi, upd ? uint32_t(a.B) : 0u, uint32_t(f)) : uint8_t(upd);
            if (at) {
                ld_upd -= k_upd;
                --ld_zi;
            }
        }
    };
    // the smoothed row against its fix
    auto em_fix = [&](const T (&z)[D], uint8_t use) {
        if constexpr (EM) {
            const bool app = use != 0;
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const T e = z[i] - sp[i];
                const T term = fmaT(e, e, spp[i]);
                em.r[i] += app ? term : T(0);
            }
            em.nfix += app ? 1 : 0;
        }
    };

    // row T - 1: the filtered row itself
    {
        T x[N], P[NP];
        load_xP(T_ - 1, x, P);
        T z_last[D];
        uint8_t use_last = 0;
        if constexpr (EM) load_z(T_ - 1, true, z_last, use_last);
        __builtin_amdgcn_s_waitcnt(0);
        bool nan = false;
#pragma unroll
        for (int i = 0; i < N; ++i) nan = nan || x[i] != x[i];
#pragma unroll
        for (int k = 0; k < NP; ++k) nan = nan || P[k] != P[k];
#pragma unroll
        for (int i = 0; i < D; ++i) {
            sp[i] = x[i];
            sv[i] = x[D + i];
            spp[i] = P[3 * i];
            spv[i] = P[3 * i + 1];
            svv[i] = P[3 * i + 2];
        }
        if (nan) poison();
        store_row(T_ - 1);
        if constexpr (EM) em_fix(z_last, use_last);
    }

    // backward steps; step s is row t = T - 2 - s (past the end: row 0 again).  EM with the initial
    // row: one more, t = -1, whose filtered row is (init_x, init_P)
    const int n = EM ? T_ - 1 + (has_init ? 1 : 0) : T_ - 1;
    if (n > 0) {
        T dt = T(a.dt);
        T hdt2 = T(0.5) * dt * dt;
        T qp = T(q_pos * a.dt), qv = T(q_vel * a.dt);
        using Row = std::conditional_t<EM, SmoothRowEm<D>, SmoothRow<D>>;
        auto load = [&](int s, Row& in) {
            const int t = T_ - 2 - (s < n ? s : n - 1);
            if constexpr (EM) {
                // wave-uniform selects: the initial row is one record row of its own
                const void* bx = t < 0 ? ka.init_x : a.filt_x;
                const void* bP = t < 0 ? ka.init_P : a.filt_P;
                const int tr = t < 0 ? 0 : t;
#pragma unroll
                for (int i = 0; i < N; ++i) in.x[i] = ldb_stream(bx, int64_t(tr) * N + i, rb, off, T(0));
#pragma unroll
                for (int k = 0; k < NP; ++k) in.P[k] = ldb_stream(bP, int64_t(tr) * NP + k, rb, off, T(0));
                load_z(t, s < n, in.z, in.use);
            } else {
                load_xP(t, in.x, in.P);
            }
#pragma unroll
            for (int i = 0; i < D; ++i) in.u[i] = ldb_stream(a.u, int64_t(t + 1) * D + i, rb_u, off, T(0));
        };
        // EM: the smoothed row before step 0
        auto store_init = [&]() {
            if constexpr (EM) {
                const uint32_t rb_ix = ka.sm_init_x != nullptr ? rb : 0u;  // absent outputs: stores dropped
                const uint32_t rb_iP = ka.sm_init_P != nullptr ? rb : 0u;
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    stb_rec(ka.sm_init_x, i, rb_ix, off, sp[i]);
                    stb_rec(ka.sm_init_x, D + i, rb_ix, off, sv[i]);
                }
#pragma unroll
                for (int i = 0; i < D; ++i) {
                    stb_rec(ka.sm_init_P, 3 * i, rb_iP, off, spp[i]);
                    stb_rec(ka.sm_init_P, 3 * i + 1, rb_iP, off, spv[i]);
                    stb_rec(ka.sm_init_P, 3 * i + 2, rb_iP, off, svv[i]);
                }
            }
        };
        auto step = [&](int s, const Row& in) {
            const int t = T_ - 2 - s;
            if (has_dts) {  // wave-uniform: the forward step t + 1's dt, in its expressions
                const double dtd = a.dt_steps[t + 1];
                dt = T(dtd);
                hdt2 = T(0.5) * dt * dt;
                qp = T(q_pos * dtd);
                qv = T(q_vel * dtd);
            }
            // EM: a transition of no duration carries no noise and is not counted (wave-uniform)
            bool em_count = false;
            T em_inv_d = T(0);
            if constexpr (EM) {
                const double d_em = has_dts ? a.dt_steps[t + 1] : a.dt;
                em_count = d_em != 0.0;
                em_inv_d = T(1) / T(d_em);
                em.ntrans += em_count ? 1 : 0;
            }
            bool bad = false;
#pragma unroll
            for (int i = 0; i < N; ++i) bad = bad || in.x[i] != in.x[i];
#pragma unroll
            for (int k = 0; k < NP; ++k) bad = bad || in.P[k] != in.P[k];
#pragma unroll
            for (int i = 0; i < D; ++i) bad = bad || in.u[i] != in.u[i];
#pragma unroll
            for (int i = 0; i < D; ++i) {
                const T fx = in.x[i], fv = in.x[D + i];
                const T fpp = in.P[3 * i], fpv = in.P[3 * i + 1], fvv = in.P[3 * i + 2];
                // predict: cv_rec_kernel's lines on the filtered row
                const T px = fmaT(hdt2, in.u[i], fmaT(dt, fv, fx));
                const T pvx = fmaT(dt, in.u[i], fv);
                const T bn = fmaT(dt, fvv, fpv);
                T ppp = fmaT(dt, bn + fpv, fpp);
                ppp += qp;
                const T ppv = bn;
                const T pvv = fvv + qv;
                // P_f F^T = [[fpp + dt fpv, fpv], [fpv + dt fvv, fvv]]
                const T a00 = fmaT(dt, fpv, fpp);
                // P_p = L D L^T (unit lower L); the two pivots are divided by exactly
                const T d0 = ppp;
                const T i0 = T(1) / d0;
                const T l10 = ppv * i0;
                const T v0 = l10 * d0;
                const T d1 = fmaT(-l10, v0, pvv);
                const T i1 = T(1) / d1;
                bad = bad || !(d0 > T(0) && d1 > T(0));
                // C row r solves P_p c = (row r of P_f F^T)^T
                const T w01 = fmaT(-l10, a00, fpv);
                const T c01 = w01 * i1;
                const T c00 = fmaT(-l10, c01, a00 * i0);
                const T w11 = fmaT(-l10, bn, fvv);
                const T c11 = w11 * i1;
                const T c10 = fmaT(-l10, c11, bn * i0);
                const T dx0 = sp[i] - px, dx1 = sv[i] - pvx;
                const T D00 = spp[i] - ppp, D01 = spv[i] - ppv, D11 = svv[i] - pvv;
                if constexpr (EM) {
                    if (em_count) {
                        // J row r solves P_p j = (row r of Q d)^T, Q d = diag(qp, qv)
                        const T j01 = (-l10 * qp) * i1;
                        const T j00 = fmaT(-l10, j01, qp * i0);
                        const T j11 = qv * i1;
                        const T j10 = -l10 * j11;
                        const T ew0 = fmaT(j01, dx1, j00 * dx0), ew1 = fmaT(j11, dx1, j10 * dx0);
                        const T jd00 = fmaT(j01, D01, j00 * D00), jd01 = fmaT(j01, D11, j00 * D01);
                        const T jd10 = fmaT(j11, D01, j10 * D00), jd11 = fmaT(j11, D11, j10 * D01);
                        const T var0 = fmaT(jd01, j01, fmaT(jd00, j00, qp));
                        const T var1 = fmaT(jd11, j11, fmaT(jd10, j10, qv));
                        em.qp += fmaT(ew0, ew0, var0) * em_inv_d;
                        em.qv += fmaT(ew1, ew1, var1) * em_inv_d;
                    }
                }
                sp[i] = fmaT(c01, dx1, fmaT(c00, dx0, fx));
                sv[i] = fmaT(c11, dx1, fmaT(c10, dx0, fv));
                const T cd00 = fmaT(c01, D01, c00 * D00), cd01 = fmaT(c01, D11, c00 * D01);
                const T cd10 = fmaT(c11, D01, c10 * D00), cd11 = fmaT(c11, D11, c10 * D01);
                spp[i] = fmaT(cd01, c01, fmaT(cd00, c00, fpp));
                spv[i] = fmaT(cd01, c11, fmaT(cd00, c10, fpv));
                svv[i] = fmaT(cd11, c11, fmaT(cd10, c10, fvv));
            }
            if (bad || st != 0) poison();
            if constexpr (EM) {
                if (t < 0) {  // wave-uniform
                    store_init();
                } else {
                    store_row(t);
                    em_fix(in.z, in.use);
                }
            } else {
                store_row(t);
            }
        };
        Row buf[DEPTH];
#pragma unroll
        for (int j = 0; j < DEPTH - 1; ++j) load(j, buf[j]);
        __builtin_amdgcn_s_waitcnt(0);
        int s = 0;
        for (; s + DEPTH <= n; s += DEPTH) {
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
                load(s + j + DEPTH - 1, buf[(j + DEPTH - 1) % DEPTH]);
                step(s + j, buf[j]);
            }
        }
#pragma unroll
        for (int j = 0; j < DEPTH - 1; ++j)
            if (s + j < n) step(s + j, buf[j]);
    }
    if (a.sm_status) a.sm_status[f] = st;
    if constexpr (EM) {
        // rows KF_EM_*: a filter that failed keeps its counts only
        const uint32_t rb_em = ka.em != nullptr ? rb : 0u;
        const bool good = st == 0;
        const double nanv = quiet_nan<double>();
        stb(ka.em, kEmNTrans, rb_em, off, double(em.ntrans));
        stb(ka.em, kEmQPos, rb_em, off, good ? em.qp : nanv);
        stb(ka.em, kEmQVel, rb_em, off, good ? em.qv : nanv);
        stb(ka.em, kEmNFix, rb_em, off, double(em.nfix));
#pragma unroll
        for (int i = 0; i < D; ++i) stb(ka.em, kEmR + i, rb_em, off, good ? em.r[i] : nanv);
    }
}

template <int D, typename T>
void launch_rec_t(const CvRecArgs& a, dim3 grid, hipStream_t st) {
    // the inputs alone choose the arithmetic's form (GENERAL), never which records are asked for
    const bool general = a.run.dt_steps != nullptr || a.run.u == nullptr || a.run.mask != nullptr;
    const bool all_rec = a.run.traj != nullptr && a.cov != nullptr && a.run.logdet != nullptr;
    if (general) cv_rec_kernel<D, T, 8, true, true><<<grid, kBlock, 0, st>>>(a);
    else if (all_rec) cv_rec_kernel<D, T, 8, false, false><<<grid, kBlock, 0, st>>>(a);
    else cv_rec_kernel<D, T, 8, false, true><<<grid, kBlock, 0, st>>>(a);
}

// kf_run_scores' instantiations: PARAMS and SCORED both on and every record optional, one per
// input shape; a NULL consts, track or scores is a wave-uniform select or a zero-length row
#ifndef KF_CV_SCORES_DEPTH
#define KF_CV_SCORES_DEPTH 4
#endif
constexpr int kCvScoresDepth = KF_CV_SCORES_DEPTH;  // their input ring (the depth changes no bit)

template <int D, typename T>
void launch_scores_t(const CvScoreArgs& a, dim3 grid, hipStream_t st) {
    const CvArgs& r = a.rec.run;
    const bool general = r.dt_steps != nullptr || r.u == nullptr || r.mask != nullptr;  // as launch_rec_t
    if (general) cv_rec_kernel<D, T, kCvScoresDepth, true, true, true, true, CvScoreArgs><<<grid, kBlock, 0, st>>>(a);
    else cv_rec_kernel<D, T, kCvScoresDepth, false, true, true, true, CvScoreArgs><<<grid, kBlock, 0, st>>>(a);
}

}  // namespace

hipError_t launch_cv_rec(int axes, bool f64, const CvRecArgs& a, hipStream_t stream) {
    if (a.run.B <= 0 || a.run.T <= 0 || (axes != 2 && axes != 3)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.run.B + kBlock - 1) / kBlock));
    if (axes == 2) {
        if (f64) launch_rec_t<2, double>(a, grid, stream);
        else launch_rec_t<2, float>(a, grid, stream);
    } else {
        if (f64) launch_rec_t<3, double>(a, grid, stream);
        else launch_rec_t<3, float>(a, grid, stream);
    }
    return hipGetLastError();
}

hipError_t launch_cv_scores(int axes, bool f64, const CvScoreArgs& a, hipStream_t stream) {
    const CvArgs& r = a.rec.run;
    if (r.B <= 0 || r.T <= 0 || (axes != 2 && axes != 3)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((r.B + kBlock - 1) / kBlock));
    if (axes == 2) {
        if (f64) launch_scores_t<2, double>(a, grid, stream);
        else launch_scores_t<2, float>(a, grid, stream);
    } else {
        if (f64) launch_scores_t<3, double>(a, grid, stream);
        else launch_scores_t<3, float>(a, grid, stream);
    }
    return hipGetLastError();
}

hipError_t launch_cv_smooth_params(int axes, const CvSmoothParamArgs& p, hipStream_t stream) {
    const CvSmoothArgs& a = p.smooth;
    if (a.B <= 0 || a.T <= 0 || (axes != 2 && axes != 3) || !a.filt_x || !a.filt_P) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.B + kBlock - 1) / kBlock));
    if (axes == 2) cv_smooth_kernel<2, kCvSmoothDepth, true, CvSmoothParamArgs><<<grid, kBlock, 0, stream>>>(p);
    else cv_smooth_kernel<3, kCvSmoothDepth, true, CvSmoothParamArgs><<<grid, kBlock, 0, stream>>>(p);
    return hipGetLastError();
}

// kf_smooth_run_em's instantiations: their input ring holds D values of z and the mask byte more
// per buffer and the lane 2 + D sums (the depth changes no bit).  At kf_smooth_run's depth of 4 the
// three-axis kernel needs 318 registers, one wave per SIMD; at 2 it fits two, and measured 12.15 ms
// against 12.41 with every output and 6.72 against 7.66 with the table alone (2^20 filters x 256
// steps, profiles/cv_em/cv_em_timing_depth*.log)
#ifndef KF_CV_EM_DEPTH
#define KF_CV_EM_DEPTH 2
#endif

hipError_t launch_cv_smooth_em(int axes, const CvSmoothEmArgs& e, hipStream_t stream) {
    const CvSmoothArgs& a = e.p.smooth;
    if (a.B <= 0 || a.T <= 0 || (axes != 2 && axes != 3) || !a.filt_x || !a.filt_P || e.update_every < 1)
        return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.B + kBlock - 1) / kBlock));
    if (axes == 2) cv_smooth_kernel<2, KF_CV_EM_DEPTH, true, CvSmoothEmArgs, true><<<grid, kBlock, 0, stream>>>(e);
    else cv_smooth_kernel<3, KF_CV_EM_DEPTH, true, CvSmoothEmArgs, true><<<grid, kBlock, 0, stream>>>(e);
    return hipGetLastError();
}

hipError_t launch_cv_smooth(int axes, const CvSmoothArgs& a, hipStream_t stream) {
    if (a.B <= 0 || a.T <= 0 || (axes != 2 && axes != 3) || !a.filt_x || !a.filt_P) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.B + kBlock - 1) / kBlock));
    if (axes == 2) cv_smooth_kernel<2, kCvSmoothDepth><<<grid, kBlock, 0, stream>>>(a);
    else cv_smooth_kernel<3, kCvSmoothDepth><<<grid, kBlock, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace kfmi

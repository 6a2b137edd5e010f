// gfx950 kernels for the reference's chain-structured GPS+IMU models on per-filter event
// streams — KF_MODEL_REF15 (kf_workers.py:493-614) and KF_MODEL_REF8 (hw5_2.py:219-311) — and
// the brute-force combination search and sensor scheduling built on the 15-state one
// (kf_workers.py:22-213, 826-957, 1218-1392).
//
// Structure exploited (exact, not an approximation): F(dt) (kf_workers.py:500-516,
// hw5_2.py:221-230) couples a state only within its axis chain (pos_i, vel_i, acc_i) or
// (att_i, rate_i); Q, R_gps, R_imu and the reference's P0 are diagonal; H_gps selects pos_i and
// H_imu = I.  So every covariance reachable from a diagonal P0 is block-diagonal — 3x3
// (pos, vel, acc) blocks and 2x2 (att, rate) blocks — and the reference's own dense arithmetic
// keeps the off-block entries at exactly 0.0 (checked on its outputs, tests/golden/ref15_*.npz).
// A lane therefore runs small chain filters: REF15 = 3 pva + 3 aw chains (27 covariance entries
// instead of 120), REF8 = 2 pva (x, y) + 1 aw (theta) chain (15 instead of 36); same numbers.
//
// Block-packed covariance rows ([NBLK][B] in HBM):
//   rows 6c .. 6c+5 : pva chain c upper triangle (pp pv pa vv va aa), c = 0..NP-1
//   rows 6NP+3c .. 6NP+3c+2 : aw chain c upper triangle (tt tw ww), c = 0..NA-1
// State x [N][B] in the reference's order.
//
// This header is the model layer of the units kf_ref_lane.hip, kf_ref_search.hip, kf_ref_stream.hip,
// kf_ref_scheduler.hip and kf_ref_schedule_search.hip, and through kf_ref_chainlane.h of
// kf_ref_chain.hip and kf_ref_sweep.hip: the constants, M15 / M8, the
// noise tables, Chains, FilterGate, the few declarations that two families share and the launchers'
// dispatch macros.  It declares in an anonymous namespace, as the units' kernels do, so only those
// units include it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "kf_common.h"
#include "kf_internal.h"

namespace kfmi {
namespace {

// Read-only device tables (the handle's custom constants, a search's events and binomials) read
// through the constant address space: a wave-uniform entry then becomes a scalar load.  Through a
// generic pointer the compiler cannot prove that a kernel's own stores leave them alone, so it
// loads them with vector loads, whose vmcnt wait also waits for every store issued before them
// (on gfx950 vmcnt counts loads and stores, in order).  Every such table is written by the host
// before the launch and never by a kernel.
template <typename T>
__device__ __forceinline__ __attribute__((address_space(4))) const T* ro(const T* p) {
    return (__attribute__((address_space(4))) const T*)p;
}
typedef __attribute__((address_space(4))) const double ro_double;
typedef __attribute__((address_space(4))) const uint64_t ro_u64;

using namespace dev;

constexpr int kGps = 0, kImu = 1;  // KF_EVENT_GPS / KF_EVENT_IMU; 2 = predict only, 255 = none
// Newton steps on the update's pivot reciprocals (see sel_update)
constexpr int kRefNewton = 1;
// Covariance update of the reference models.  fp64 takes the reference's own form
// P = (I - K H) P (kf_workers.py:711, hw5_2.py:358, 376) over the packed upper triangle, its
// observed rows as K R (sel_update_nv: the same value without 1 - K's cancellation); fp32 keeps
// Joseph's, which the fp32 parity gate needs (the simple form drifts there).
// KF_REF_JOSEPH_F64=1 builds fp64 with Joseph too (the A/B arm).
#ifndef KF_REF_JOSEPH_F64
#define KF_REF_JOSEPH_F64 0
#endif
template <typename T>
constexpr bool kRefJoseph = sizeof(T) == 4 || KF_REF_JOSEPH_F64 != 0;
// The IMU pseudo-measurement's H = I chain updates take P = K R (sel_update_nv's GAIN_R: the
// same value as (I - K)P, without its cancellation), in both precisions; KF_REF_GAIN_R=0 builds
// the A/B arm without it (fp64: the cancelling P - K P on every row; fp32: Joseph's).
#ifndef KF_REF_GAIN_R
#define KF_REF_GAIN_R 1
#endif
constexpr bool kRefGainR = KF_REF_GAIN_R != 0;

// Noise constants shared by both reference models (kf_workers.py:519-544, 581-614;
// hw5_2.py:233-251, 280-304).
constexpr double kQPos = 5.0, kQAtt = 0.05, kQVel = 1.0, kQRate = 0.1, kQAcc = 2.0;
constexpr double kRGps = 3.0;
constexpr double kRPos = 50.0, kRAtt = 0.05, kRVel = 10.0, kRRate = 0.1, kRAcc = 100.0;

// KF_MODEL_REF15: x = (pos xyz, att rpy, vel xyz, rate xyz, acc xyz) (kf_workers.py:493-517).
struct M15 {
    static constexpr int N = 15, NP = 3, NA = 3, NTRAJ = 6, NBLK = 27;
    __device__ static constexpr int pva(int c, int k) { return c + 6 * k; }          // (i, 6+i, 12+i)
    __device__ static constexpr int aw(int c, int k) { return 3 + c + 6 * k; }       // (3+i, 9+i)
    __device__ static constexpr int imu_acc(int c) { return 6 + c; }                 // ax, ay, az
    __device__ static constexpr int imu_att(int c) { return c; }                     // roll, pitch, yaw
    __device__ static constexpr int imu_rate(int c) { return 3 + c; }                // wx, wy, wz
    static constexpr double P0Pos = 10000.0, P0Att = 1000.0, P0Vel = 1000.0, P0Rate = 1000.0,
                            P0Acc = 10000.0;  // kf_workers.py:651
};

// KF_MODEL_REF8: x = (x, y, theta, vx, vy, theta_dot, ax, ay) (hw5_2.py:219-231); the IMU
// pseudo-measurement takes yaw as theta and wz as theta_dot (hw5_2.py:355-362).
struct M8 {
    static constexpr int N = 8, NP = 2, NA = 1, NTRAJ = 3, NBLK = 15;
    __device__ static constexpr int pva(int c, int k) { return c + 3 * k; }          // (i, 3+i, 6+i)
    __device__ static constexpr int aw(int, int k) { return 2 + 3 * k; }             // (2, 5)
    __device__ static constexpr int imu_acc(int c) { return 6 + c; }                 // ax, ay
    __device__ static constexpr int imu_att(int) { return 2; }                       // yaw
    __device__ static constexpr int imu_rate(int) { return 5; }                      // wz
    static constexpr double P0Pos = 1000.0, P0Att = 100.0, P0Vel = 100.0, P0Rate = 100.0,
                            P0Acc = 1000.0;  // hw5_2.py:317-326
};

// Noise constants of a chain.  CUSTOM = false: the reference's, compile-time literals (the
// default, and the code every bench row runs); CUSTOM = true: a caller's diagonal Q rates, R_imu,
// R_gps and P0 per state (kf_params -> RefConsts, the handle's device copy at kc), read by
// wave-uniform scalar loads.  Both give Chains the same operations in the same order.
template <bool CUSTOM, class M, typename T>
__device__ __forceinline__ void pva_noise(const RefConsts* kc, int c, T (&q)[3], T (&r)[6], T& rg) {
    if constexpr (CUSTOM) {
#pragma unroll
        for (int k = 0; k < 3; ++k) q[k] = T(ro(kc)->q[M::pva(c, k)]);
        r[0] = T(ro(kc)->r_imu[M::pva(c, 0)]);
        r[3] = T(ro(kc)->r_imu[M::pva(c, 1)]);
        r[5] = T(ro(kc)->r_imu[M::pva(c, 2)]);
        rg = T(ro(kc)->r_gps[c]);
    } else {
        q[0] = T(kQPos);
        q[1] = T(kQVel);
        q[2] = T(kQAcc);
        r[0] = T(kRPos);
        r[3] = T(kRVel);
        r[5] = T(kRAcc);
        rg = T(kRGps);
    }
    r[1] = r[2] = r[4] = T(0);
}
template <bool CUSTOM, class M, typename T>
__device__ __forceinline__ void aw_noise(const RefConsts* kc, int c, T (&q)[2], T (&r)[3]) {
    if constexpr (CUSTOM) {
        q[0] = T(ro(kc)->q[M::aw(c, 0)]);
        q[1] = T(ro(kc)->q[M::aw(c, 1)]);
        r[0] = T(ro(kc)->r_imu[M::aw(c, 0)]);
        r[2] = T(ro(kc)->r_imu[M::aw(c, 1)]);
    } else {
        q[0] = T(kQAtt);
        q[1] = T(kQRate);
        r[0] = T(kRAtt);
        r[2] = T(kRRate);
    }
    r[1] = T(0);
}

template <typename T, class M, bool CUSTOM = false>
struct Chains {
    T x[M::N];
    T pva[M::NP][6];  // per chain: (pos, vel, acc) packed upper 3x3
    T aw[M::NA][3];   // per chain: (att, rate) packed upper 2x2
    const RefConsts* kc = nullptr;  // CUSTOM: the noise constants (kf_params)
    // Chain predict x = F x, P = F P F^T + Q for a block whose F row i is
    // e_i + dt e_{i+1} + dt^2/2 e_{i+2} (kf_workers.py:500-516).
    template <int NB>
    __device__ static __forceinline__ void chain_predict(T (&xb)[NB], T (&Pb)[NB * (NB + 1) / 2], T dt,
                                                         const T (&q)[NB]) {
        const T c[3] = {T(1), dt, T(0.5) * dt * dt};
        // the d / e loops run a constant 2 trips with a compile-time guard: a trip count of
        // min(NB - i, 3) - 1 was left as a runtime loop with indexed register reads (s_set_gpr_idx)
        T xn[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            T s = xb[i];
#pragma unroll
            for (int d = 1; d < 3; ++d)
                if (i + d < NB) s = fmaT(c[d], xb[i + d], s);
            xn[i] = s;
        }
        T FP[NB][NB];
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = 0; j < NB; ++j) {
                T s = Pb[tri<NB>(i, j)];
#pragma unroll
                for (int d = 1; d < 3; ++d)
                    if (i + d < NB) s = fmaT(c[d], Pb[tri<NB>(i + d, j)], s);
                FP[i][j] = s;
            }
#pragma unroll
        for (int i = 0; i < NB; ++i)
#pragma unroll
            for (int j = i; j < NB; ++j) {
                T s = FP[i][j];
#pragma unroll
                for (int e = 1; e < 3; ++e)
                    if (j + e < NB) s = fmaT(FP[i][j + e], c[e], s);
                Pb[tri<NB>(i, j)] = (i == j) ? s + q[i] * dt : s;
            }
#pragma unroll
        for (int i = 0; i < NB; ++i) xb[i] = xn[i];
    }

    __device__ __forceinline__ void predict(T dt) {
#pragma unroll
        for (int c = 0; c < M::NP; ++c) {
            T qpva[3], r[6], rg;
            pva_noise<CUSTOM, M>(kc, c, qpva, r, rg);
            T xb[3];
            get_pva(c, xb);
            chain_predict<3>(xb, pva[c], dt, qpva);
            put_pva(c, xb);
        }
#pragma unroll
        for (int c = 0; c < M::NA; ++c) {
            T qaw[2], r[3];
            aw_noise<CUSTOM, M>(kc, c, qaw, r);
            T xa[2];
            get_aw(c, xa);
            chain_predict<2>(xa, aw[c], dt, qaw);
            put_aw(c, xa);
        }
    }

    __device__ __forceinline__ void get_pva(int c, T (&xb)[3]) const {
#pragma unroll
        for (int k = 0; k < 3; ++k) xb[k] = x[M::pva(c, k)];
    }
    __device__ __forceinline__ void put_pva(int c, const T (&xb)[3]) {
#pragma unroll
        for (int k = 0; k < 3; ++k) x[M::pva(c, k)] = xb[k];
    }
    __device__ __forceinline__ void get_aw(int c, T (&xa)[2]) const {
#pragma unroll
        for (int k = 0; k < 2; ++k) xa[k] = x[M::aw(c, k)];
    }
    __device__ __forceinline__ void put_aw(int c, const T (&xa)[2]) {
#pragma unroll
        for (int k = 0; k < 2; ++k) x[M::aw(c, k)] = xa[k];
    }

    // GPS fix (kf_workers.py:694-697, hw5_2.py:341-349): H selects pos_c in each (pos, vel,
    // acc) chain, R = 3; z = (easting, northing[, altitude]).
    template <bool POISON = true>
    __device__ __forceinline__ bool update_gps(const T (&z)[3]) {
        bool ok = true;
#pragma unroll
        for (int c = 0; c < M::NP; ++c) {
            T q[3], r[6], rg;
            pva_noise<CUSTOM, M>(kc, c, q, r, rg);
            const T R[1] = {rg};
            T xb[3];
            get_pva(c, xb);
            const T zb[1] = {z[c]};
            ok = sel_update<3, 1, true, T, kRefNewton, POISON, kRefJoseph<T>, kRefGainR>(xb, pva[c], zb, R) && ok;
            put_pva(c, xb);
        }
        return ok;
    }

    // IMU pseudo-measurement (kf_workers.py:698-706, hw5_2.py:352-366): Z from the PREDICTED
    // state and the raw sample, H = I, R = diag(50, 0.05, 10, 0.1, 100 per group).  imu = (roll,
    // pitch, yaw, wx, wy, wz, ax, ay, az).
    // `imu` is any indexable payload: a register array, or an LDS image (ref_events_lds_kernel)
    template <bool POISON = true, class Pay>
    __device__ __forceinline__ bool update_imu(const Pay& imu, T dt) {
        bool ok = true;
#pragma unroll
        for (int c = 0; c < M::NP; ++c) {
            T q[3], Rp[6], rg;
            pva_noise<CUSTOM, M>(kc, c, q, Rp, rg);
            T xb[3];
            get_pva(c, xb);
            const T a = imu[M::imu_acc(c)];
            const T V = fmaT(a, dt, xb[1]);   // V = x_v + a dt
            const T X = fmaT(V, dt, xb[0]);   // X = x_p + V dt
            const T zb[3] = {X, V, a};
            ok = sel_update<3, 3, true, T, kRefNewton, POISON, kRefJoseph<T>, kRefGainR>(xb, pva[c], zb, Rp) && ok;
            put_pva(c, xb);
        }
#pragma unroll
        for (int c = 0; c < M::NA; ++c) {
            T q[2], Ra[3];
            aw_noise<CUSTOM, M>(kc, c, q, Ra);
            T xa[2];
            get_aw(c, xa);
            const T za[2] = {imu[M::imu_att(c)], imu[M::imu_rate(c)]};
            ok = sel_update<2, 2, true, T, kRefNewton, POISON, kRefJoseph<T>, kRefGainR>(xa, aw[c], za, Ra) && ok;
            put_aw(c, xa);
        }
        return ok;
    }

    // slogdet of the full P = sum over the chain blocks (kf_workers.py:716-717): the product of
    // the blocks' determinants, division-free per block (det3_scaled / det2) and one reciprocal
    // for the pva pivots; fp32 renormalises after every block (three pva blocks reach 1e48).
    __device__ __forceinline__ T logdet() const {
        int ex;
        const T prod = det_mant(ex);
        const T ld = log_mant(prod, ex);
        return prod == prod ? ld : quiet_nan<T>();
    }
    // the same determinant before its log: mantissa in [0.5, 1) (NaN unless positive definite)
    // times 2^ex
    __device__ __forceinline__ T det_mant(int& ex) const {
        constexpr bool kNarrow = sizeof(T) == 4;
        T num = T(1), den = T(1);
        ex = 0;
        bool ok = true;
#pragma unroll
        for (int c = 0; c < M::NP; ++c) {
            det3_scaled<T>(pva[c], num, den, ok);
            if (kNarrow || c == M::NP - 1) renorm(num, ex);
        }
#pragma unroll
        for (int c = 0; c < M::NA; ++c) {
            det2<T>(aw[c], num, ok);
            if (kNarrow) renorm(num, ex);
        }
        T prod = num * rcp_nr<kRefNewton>(den);
        renorm(prod, ex);
        return ok ? prod : quiet_nan<T>();
    }

    __device__ __forceinline__ void reset_cov() {
        const T p[6] = {T(M::P0Pos), T(0), T(0), T(M::P0Vel), T(0), T(M::P0Acc)};
        const T w[3] = {T(M::P0Att), T(0), T(M::P0Rate)};
#pragma unroll
        for (int c = 0; c < M::NP; ++c)
#pragma unroll
            for (int k = 0; k < 6; ++k) pva[c][k] = p[k];
#pragma unroll
        for (int c = 0; c < M::NA; ++c)
#pragma unroll
            for (int k = 0; k < 3; ++k) aw[c][k] = w[k];
        if constexpr (CUSTOM) {  // P0 = diag(p0) in the model's state order
#pragma unroll
            for (int c = 0; c < M::NP; ++c) {
                pva[c][0] = T(ro(kc)->p0[M::pva(c, 0)]);
                pva[c][3] = T(ro(kc)->p0[M::pva(c, 1)]);
                pva[c][5] = T(ro(kc)->p0[M::pva(c, 2)]);
            }
#pragma unroll
            for (int c = 0; c < M::NA; ++c) {
                aw[c][0] = T(ro(kc)->p0[M::aw(c, 0)]);
                aw[c][2] = T(ro(kc)->p0[M::aw(c, 1)]);
            }
        }
    }

    // block-packed covariance row r (see the file comment)
    __device__ __forceinline__ T& blk(int r) { return r < 6 * M::NP ? pva[r / 6][r % 6] : aw[(r - 6 * M::NP) / 3][(r - 6 * M::NP) % 3]; }
    __device__ __forceinline__ T blk(int r) const { return r < 6 * M::NP ? pva[r / 6][r % 6] : aw[(r - 6 * M::NP) / 3][(r - 6 * M::NP) % 3]; }

    __device__ __forceinline__ void load(const void* xbase, const void* Pbase, uint32_t rb, uint32_t off) {
#pragma unroll
        for (int i = 0; i < M::N; ++i) x[i] = ldb<T>(xbase, i, rb, off);
#pragma unroll
        for (int r = 0; r < M::NBLK; ++r) blk(r) = ldb<T>(Pbase, r, rb, off);
    }

    __device__ __forceinline__ void store(void* xbase, void* Pbase, uint32_t rb, uint32_t off) const {
#pragma unroll
        for (int i = 0; i < M::N; ++i) stb(xbase, i, rb, off, x[i]);
        store_cov(Pbase, 0, rb, off);
    }

    // covariance rows at row offset r0 of a [.][B] array (r0 = t * NBLK for a per-step record)
    __device__ __forceinline__ void store_cov(void* Pbase, int64_t r0, uint32_t rb, uint32_t off) const {
#pragma unroll
        for (int r = 0; r < M::NBLK; ++r) stb(Pbase, r0 + r, rb, off, blk(r));
    }

    __device__ __forceinline__ void fill_nan() {
#pragma unroll
        for (int i = 0; i < M::N; ++i) x[i] = quiet_nan<T>();
#pragma unroll
        for (int r = 0; r < M::NBLK; ++r) blk(r) = quiet_nan<T>();
    }

    // One event of the reference loop (kf_workers.py:682-717): predict over dt, then the GPS or
    // IMU update; with `gate`, the update only when logdet(P_pred) > threshold
    // (run_adaptive_threshold_kalman_filter, kf_workers.py:1023-1025).  Returns whether the
    // update was applied; `ok` turns false on a non-positive-definite S.
    // POISON = false for callers that fill the filter with NaN when `ok` turns false
    template <bool POISON = true, class Pay>
    __device__ __forceinline__ bool event(int type, T dt, const Pay& pay, bool gate, T threshold, bool& ok) {
        predict(dt);
        bool apply = (type == kGps || type == kImu);
        if (gate && apply) apply = logdet() > threshold;
        if (apply) {
            if (type == kGps) {
                const T z[3] = {pay[0], pay[1], pay[2]};  // (easting, northing, altitude)
                ok = update_gps<POISON>(z) && ok;
            } else {
                ok = update_imu<POISON>(pay, dt) && ok;
            }
        }
        return apply;
    }
};

// GATES (kf_run_events_gates): filter f's update is gated by its own a.thresholds[f], in the
// sweep's conventions (gate_of); the instantiations without it are kf_run_events' as before.
template <typename T>
struct FilterGate {
    bool on;  // the gate is evaluated (false: every event updates)
    T thr;
};
template <typename T>
__device__ __forceinline__ FilterGate<T> gate_of(const double* thresholds, int64_t f) {
    const double t = thresholds[f];
    // -inf is "always update": the gate is not evaluated; +inf and NaN fail every comparison
    return FilterGate<T>{t != -__builtin_inf(), T(t)};
}

// What more than one family reads.
// s_waitcnt immediates; read by the lane unit's LDS kernel and the scheduler's LDS kernels
constexpr int vmcnt_imm(int n) { return (n & 15) | (7 << 4) | (15 << 8) | ((n >> 4) << 14); }
constexpr int lgkmcnt0_imm = 15 | (7 << 4) | (0 << 8) | (3 << 14);  // LDS reads drained, vmcnt untouched

// a search's candidate events at most; read by the combos and search kernels and their launchers
constexpr int kMaxEvents = 64;

// the 15-state lane; read by the combos, search and scheduler kernels
template <typename T, bool CUSTOM = false>
using Ref15 = Chains<T, M15, CUSTOM>;

}  // namespace

}  // namespace kfmi

// kernel<..., CUSTOM> for a launch: the reference's constants (kc == nullptr) or the handle's
#define KF_CUSTOM_DISPATCH(kc, ...)         \
    do {                                    \
        if (kc) {                           \
            constexpr bool CUSTOM = true;   \
            __VA_ARGS__;                    \
        } else {                            \
            constexpr bool CUSTOM = false;  \
            __VA_ARGS__;                    \
        }                                   \
    } while (0)

// the statement with the compile-time bool NAME in scope, taken from a runtime condition (a
// kernel's other template flags: SYM, GATES, ...)
#define KF_BOOL_DISPATCH(cond, NAME, ...)  \
    do {                                   \
        if (cond) {                        \
            constexpr bool NAME = true;    \
            __VA_ARGS__;                   \
        } else {                           \
            constexpr bool NAME = false;   \
            __VA_ARGS__;                   \
        }                                  \
    } while (0)

// the statement with M = M15 / M8 and T = double / float in scope (model is 15 or 8: the
// launchers check); KF_REF_DISPATCH adds CUSTOM
#define KF_DTYPE_DISPATCH(f64, ...) \
    do {                            \
        if (f64) {                  \
            using T = double;       \
            __VA_ARGS__;            \
        } else {                    \
            using T = float;        \
            __VA_ARGS__;            \
        }                           \
    } while (0)
#define KF_MODEL_DISPATCH(model, f64, ...)          \
    do {                                            \
        if ((model) == 15) {                        \
            using M = M15;                          \
            KF_DTYPE_DISPATCH(f64, __VA_ARGS__);    \
        } else {                                    \
            using M = M8;                           \
            KF_DTYPE_DISPATCH(f64, __VA_ARGS__);    \
        }                                           \
    } while (0)
#define KF_REF_DISPATCH(model, f64, kc, ...) KF_CUSTOM_DISPATCH(kc, KF_MODEL_DISPATCH(model, f64, __VA_ARGS__))

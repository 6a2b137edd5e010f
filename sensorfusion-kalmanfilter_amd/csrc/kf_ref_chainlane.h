// What the 8-lanes-per-filter kernels share: the lane group's DPP exchanges, the banded gate, one
// lane's chain with its event step (ChainLane) and the input ring.  Like kf_ref_model.h it declares
// in an anonymous namespace: only kf_ref_chain.hip and kf_ref_sweep.hip include it.
#pragma once
#include "kf_ref_model.h"

namespace kfmi {
namespace {

constexpr int kGroup = 8;  // lanes per filter: one per axis chain

// Sums / ORs over the 8-lane group with DPP (a VALU-latency lane exchange, no LDS round trip):
// quad_perm [1,0,3,2] (xor 1), quad_perm [2,3,0,1] (xor 2), then row_half_mirror (lane i <-> 7-i
// within each 8 lanes), which pairs the two quads.  Every lane of the group ends with the total.
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141;
constexpr int kDppRowRor8 = 0x128;  // row_ror:8: lane l of a 16-lane row reads lane l +- 8

template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const v2u u = __builtin_bit_cast(v2u, v);
    v2u r;
    r.x = __builtin_amdgcn_mov_dpp(int(u.x), CTRL, 0xF, 0xF, false);
    r.y = __builtin_amdgcn_mov_dpp(int(u.y), CTRL, 0xF, 0xF, false);
    return __builtin_bit_cast(double, r);
}
template <int CTRL>
__device__ __forceinline__ float dpp_d(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
}

template <typename T>
__device__ __forceinline__ T group_sum(T v) {
    v += dpp_d<kDppXor1>(v);
    v += dpp_d<kDppXor2>(v);
    v += dpp_d<kDppHalfMirror>(v);
    return v;
}

__device__ __forceinline__ bool group_any(bool b) {
    int v = b ? 1 : 0;
    v |= __builtin_amdgcn_mov_dpp(v, kDppXor1, 0xF, 0xF, false);
    v |= __builtin_amdgcn_mov_dpp(v, kDppXor2, 0xF, 0xF, false);
    v |= __builtin_amdgcn_mov_dpp(v, kDppHalfMirror, 0xF, 0xF, false);
    return v != 0;
}

template <typename T>
__device__ __forceinline__ T chain_log_det(const T (&P)[6]) {
    // one 3-state chain's log det (an aw chain's inert third state has variance 1, no coupling)
    T num = T(1), den = T(1);
    int ex = 0;
    bool ok = true;
    det3_scaled<T>(P, num, den, ok);
    T prod = num * rcp_nr<kRefNewton>(den);
    renorm(prod, ex);
    const T ld = log_mant(prod, ex);
    return ok ? ld : quiet_nan<T>();
}

// chain_log_det before its log: the determinant as a mantissa in [0.5, 1) (NaN unless the
// block is positive definite) and a binary exponent
template <typename T>
__device__ __forceinline__ void chain_det_mant(const T (&P)[6], T& m, int& ex) {
    T num = T(1), den = T(1);
    bool ok = true;
    det3_scaled<T>(P, num, den, ok);
    m = num * rcp_nr<kRefNewton>(den);
    ex = 0;
    renorm(m, ex);
    m = ok ? m : quiet_nan<T>();
}

// (mantissa, exponent) product over the 8-lane group, the same DPP pattern as group_sum: every
// lane ends with the same bits (each step multiplies a pair in both orders, and x * y == y * x)
template <typename T>
__device__ __forceinline__ void group_prod(T& m, int& ex) {
    m *= dpp_d<kDppXor1>(m);
    ex += __builtin_amdgcn_mov_dpp(ex, kDppXor1, 0xF, 0xF, false);
    m *= dpp_d<kDppXor2>(m);
    ex += __builtin_amdgcn_mov_dpp(ex, kDppXor2, 0xF, 0xF, false);
    m *= dpp_d<kDppHalfMirror>(m);
    ex += __builtin_amdgcn_mov_dpp(ex, kDppHalfMirror, 0xF, 0xF, false);
}

// The adaptive gate logdet(P_pred) > threshold (kf_workers.py:1023-1025) of the chain kernel,
// decided on the group's determinant product (mantissa, binary exponent) against
// exp(threshold) (1 -+ eps); only inside that band are the logs taken, as
// group_sum(chain_log_det) > threshold, so every decision is the logs' (eps far above the logs'
// and the products' rounding: 1e-10 in f64, 1e-4 in f32).  The log is the longest part of a
// gated event's dependent chain, and a gated filter with few updates runs little else.
// Non-finite or huge thresholds take the logs every event.
template <typename T>
struct GateBand {
    T lo_m = T(0), hi_m = T(0);
    int lo_e = 0, hi_e = 0;
    bool banded = false;
    __device__ __forceinline__ void init(double thr) {
        banded = thr == thr && thr > -1e6 && thr < 1e6;
        if (!banded) return;
        const double eps = sizeof(T) == 8 ? 1e-10 : 1e-4;
        const double k = floor(thr * 1.4426950408889634);  // exp(thr) = 2^k exp(r), r in [0, ln 2)
        const double r = thr - k * 0.6931471805599453;
        int e1, e2;
        const double lo = frexp(exp(r) * (1.0 - eps), &e1), hi = frexp(exp(r) * (1.0 + eps), &e2);
        lo_m = T(lo);
        hi_m = T(hi);
        lo_e = int(k) + e1;
        hi_e = int(k) + e2;
    }
    // the gate for this lane's chain covariance P (live: a chain lane of the group)
    __device__ __forceinline__ bool open(const T (&P)[6], bool live, T thr) const {
        if (banded) {
            T m;
            int ex;
            chain_det_mant(P, m, ex);
            m = live ? m : T(1);
            ex = live ? ex : 0;
            group_prod(m, ex);
            int e;
            m = frexp(m, &e);
            ex += e;
            if (!(m > T(0))) return false;                           // NaN (a failed block) or 0: log -inf
            if (ex < lo_e || (ex == lo_e && m < lo_m)) return false;  // the logs' sum below thr
            if (ex > hi_e || (ex == hi_e && m > hi_m)) return true;   // above
        }
        return group_sum(live ? chain_log_det(P) : T(0)) > thr;
    }
};

// Inputs of one event for one lane.
template <typename T>
struct ChainIn {
    int type;
    double dt;
    T va, vb;
};

// A scored sweep's event (ref_sweep_kernel's SCORE): the track row too, the lane's own column first
template <typename T>
struct ChainInScored : ChainIn<T> {
    double track[3];
};

// What one lane of a scored sweep accumulates for its own chain, in event order: the NIS terms
// and the position error in double, and det S as a running (mantissa, exponent) product of the
// pivots in double, renormalised every update (a relative rounding per pivot, so the log taken
// once at the end is off by about 1e-16 per pivot whatever the sum's size; a log per update
// would add a rounding of the running sum each time, and ~25 VALU operations).  Branch-free and
// the same code on every lane: a lane without a chain accumulates what nobody reads, and an aw
// lane's inert third state, whose innovation is exactly 0 and whose pivot is exactly 1 + 1, adds
// 0 to the NIS and 1 to the exponent per IMU update, which the final log takes back (exactly).
struct ScoreAcc {
    int32_t ngps = 0;               // applied GPS updates (the same in every lane of a group)
    double nis[2] = {0.0, 0.0};     // this chain's sum of w_a^2 / d_a: GPS, IMU
    double ldm[2] = {1.0, 1.0};     // this chain's pivot product, mantissa ...
    int32_t lde[2] = {0, 0};        // ... and binary exponent
    int32_t npos = 0;               // events scored against the track
    double sse = 0.0;               // this axis' sum of (x - track)^2

    // one applied update of this lane's chain
    template <typename T, int M>
    __device__ __forceinline__ void add(int kind, const Innov<T, M>& in) {
        double m = ldm[kind];
#pragma unroll
        for (int a = 0; a < M; ++a) m *= double(in.d[a]);
        nis[kind] += double(in.nis);
        ldm[kind] = m;
        renorm(ldm[kind], lde[kind]);
    }
};

// Column f of a parameter sweep's constants table [2 N + NP][B] (SweepArgs::consts)
struct ConstsColumn {
    const double* table;
    int64_t B, f;
};

// The same column where there is a table, else the handle's own constants (or the literals):
// ref_smooth_kernel's EM instantiations, which take either
struct ConstsOrHandle {
    ConstsColumn col;
    const RefConsts* kc;
};

// One lane of the 8-lanes-per-filter kernels (ref_chain_kernel, ref_sweep_kernel,
// ref_chain_gated_kernel): which chain lane c of a group runs, where that chain's states, block
// rows and payload columns are, its noise constants, and the event all three kernels run.  The
// kernels keep their own address tables (state banks, record rows, stream columns).
template <typename T, class M, bool CUSTOM>
struct ChainLane {
    int c;       // lane of the group
    bool pva;    // a (pos, vel, acc) chain; otherwise an (att, rate) chain or none
    bool live;   // the lane holds a chain
    int ca;      // the chain's axis among its kind
    int xi[3];   // state indices (-1: none)
    int pr[6];   // block-packed covariance rows (-1: none)
    int ia, ib;  // payload columns: GPS position / IMU attitude, IMU acceleration / rate
    T q[3], Rimu[6], Rgps;

    __device__ __forceinline__ ChainLane(int lane, const RefConsts* kc)
        : c(lane), pva(lane < M::NP), live(lane < M::NP + M::NA), ca(pva ? lane : (live ? lane - M::NP : 0)) {
#pragma unroll
        for (int k = 0; k < 3; ++k) xi[k] = !live ? -1 : pva ? M::pva(ca, k) : (k < 2 ? M::aw(ca, k) : -1);
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const int aw_row = k == 0 ? 0 : k == 1 ? 1 : k == 3 ? 2 : -1;  // (tt tw ww) of the 3x3 packing
            pr[k] = !live ? -1 : pva ? 6 * ca + k : (aw_row < 0 ? -1 : 6 * M::NP + 3 * ca + aw_row);
        }
        ia = pva ? ca : M::imu_att(ca);
        ib = pva ? M::imu_acc(ca) : M::imu_rate(ca);
        q[0] = T(pva ? kQPos : kQAtt), q[1] = T(pva ? kQVel : kQRate), q[2] = T(pva ? kQAcc : 0.0);
        Rimu[0] = T(pva ? kRPos : kRAtt), Rimu[3] = T(pva ? kRVel : kRRate), Rimu[5] = T(pva ? kRAcc : 1.0);
        Rimu[1] = Rimu[2] = Rimu[4] = T(0);
        Rgps = T(kRGps);
        if constexpr (CUSTOM) {  // this lane's chain states (the inert third state of an aw lane keeps 0 / 1)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (xi[k] >= 0) {
                    q[k] = T(ro(kc)->q[xi[k]]);
                    Rimu[k == 0 ? 0 : k == 1 ? 3 : 5] = T(ro(kc)->r_imu[xi[k]]);
                }
            if (pva) Rgps = T(ro(kc)->r_gps[ca]);
        }
    }

    // The lane of filter f of a parameter sweep (ref_sweep_kernel's PARAMS): its chain's constants
    // from column f of the table consts [2 N + NP][B] (rows: q per state, r_imu per state, r_gps
    // per axis), converted as the CUSTOM constants are.  Plain per-lane vector loads, every one in
    // bounds: a lane without the state reads row 0 of the section and keeps the literal (an aw
    // lane's inert third state: Q = 0, R = 1).
    __device__ __forceinline__ ChainLane(int lane, const ConstsColumn& col)
        : ChainLane(lane, static_cast<const RefConsts*>(nullptr)) {
        static_assert(!CUSTOM, "the table replaces the handle's constants");
        const double* consts = col.table;
        const int64_t B = col.B, f = col.f;
        double tq[3], tr[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int row = xi[k] >= 0 ? xi[k] : 0;
            tq[k] = consts[int64_t(row) * B + f];
            tr[k] = consts[int64_t(M::N + row) * B + f];
        }
        const double tg = consts[int64_t(2 * M::N + (pva ? ca : 0)) * B + f];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (xi[k] >= 0) {
                q[k] = T(tq[k]);
                Rimu[k == 0 ? 0 : k == 1 ? 3 : 5] = T(tr[k]);
            }
        if (pva) Rgps = T(tg);
    }

    // The lane of filter f under either source (ref_smooth_kernel's EM): the table's column as
    // above or, with no table, the handle's constants converted as the CUSTOM lanes convert them
    // (kc null: the literals).  The choice is wave-uniform.
    __device__ __forceinline__ ChainLane(int lane, const ConstsOrHandle& src)
        : ChainLane(lane, static_cast<const RefConsts*>(nullptr)) {
        static_assert(!CUSTOM, "the source is chosen at run time");
        if (src.col.table) {
            const ChainLane t(lane, src.col);
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = t.q[k];
#pragma unroll
            for (int k = 0; k < 6; ++k) Rimu[k] = t.Rimu[k];
            Rgps = t.Rgps;
        } else if (src.kc) {
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (xi[k] >= 0) {
                    q[k] = T(ro(src.kc)->q[xi[k]]);
                    Rimu[k == 0 ? 0 : k == 1 ? 3 : 5] = T(ro(src.kc)->r_imu[xi[k]]);
                }
            if (pva) Rgps = T(ro(src.kc)->r_gps[ca]);
        }
    }

    // P[k] where the lane holds no row k: the identity (an aw lane's inert state has variance 1)
    static __device__ __forceinline__ T unit(int k) { return T(k == 0 || k == 3 || k == 5 ? 1 : 0); }

    // event's predict, line for line, for ref_smooth_kernel: x = F x for the NL states, P = F P F^T
    // + Q dt, F = [[1, dt, c02], [0, 1, c12], [0, 0, 1]] (c02 = c12 = 0 on an aw lane), the same
    // operations in the same order, so its P is event's P_pred bit for bit.  FP leaves with F P of
    // the covariance that came in (the smoother gain reads it).  event keeps its own copy of these
    // lines: calling this member from it compiled every chain-layout kernel to another instruction
    // stream (profiles/rts_smoother/isa_compare_predict_member.log).  Change both together.
    template <int NL>
    __device__ __forceinline__ void predict(T dt, T (&x)[NL][3], T (&P)[6], T (&FP)[3][3]) const {
        const T c02 = pva ? T(0.5) * dt * dt : T(0);
        const T c12 = pva ? dt : T(0);
#pragma unroll
        for (int v = 0; v < NL; ++v) {
            const T xn0 = fmaT(c02, x[v][2], fmaT(dt, x[v][1], x[v][0]));
            const T xn1 = fmaT(c12, x[v][2], x[v][1]);
            x[v][0] = xn0;
            x[v][1] = xn1;
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            FP[0][j] = fmaT(c02, P[tri<3>(2, j)], fmaT(dt, P[tri<3>(1, j)], P[tri<3>(0, j)]));
            FP[1][j] = fmaT(c12, P[tri<3>(2, j)], P[tri<3>(1, j)]);
            FP[2][j] = P[tri<3>(2, j)];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) {
                T s = FP[i][j];
                if (j == 0) s = fmaT(FP[i][2], c02, fmaT(FP[i][1], dt, s));
                if (j == 1) s = fmaT(FP[i][2], c12, s);
                P[tri<3>(i, j)] = (i == j) ? s + q[i] * dt : s;
            }
    }

    // One event on this lane's chain, for NL states that share the covariance: predict, the
    // adaptive gate (gated: against thr, through the group's GateBand), the GPS / IMU update,
    // the aw lane's inert-state reset, and NaN poisoning of the whole group when any of its chains
    // failed (st then kNotSpd).  Returns whether the update was applied; every lane of the group
    // must call it together (the gate and the poisoning exchange over the group).
    // SCORE (a scored sweep): an applied update also adds its chain's innovation statistics to *sc
    // (sel_update_nv's INNOV: the y, L and pivots of the update that runs anyway).
    template <int NL, bool SCORE = false>
    __device__ __forceinline__ bool event(int type, T dt, T va, T vb, bool gated, const GateBand<T>& gate, T thr,
                                          T (&x)[NL][3], T (&P)[6], int32_t& st, ScoreAcc* sc = nullptr) const {
        if (type == 255) return false;
        // predict: F = [[1, dt, c02], [0, 1, c12], [0, 0, 1]] (c02 = c12 = 0 on an aw lane)
        const T c02 = pva ? T(0.5) * dt * dt : T(0);
        const T c12 = pva ? dt : T(0);
#pragma unroll
        for (int v = 0; v < NL; ++v) {
            const T xn0 = fmaT(c02, x[v][2], fmaT(dt, x[v][1], x[v][0]));
            const T xn1 = fmaT(c12, x[v][2], x[v][1]);
            x[v][0] = xn0;
            x[v][1] = xn1;
        }
        T FP[3][3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            FP[0][j] = fmaT(c02, P[tri<3>(2, j)], fmaT(dt, P[tri<3>(1, j)], P[tri<3>(0, j)]));
            FP[1][j] = fmaT(c12, P[tri<3>(2, j)], P[tri<3>(1, j)]);
            FP[2][j] = P[tri<3>(2, j)];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) {
                T s = FP[i][j];
                if (j == 0) s = fmaT(FP[i][2], c02, fmaT(FP[i][1], dt, s));
                if (j == 1) s = fmaT(FP[i][2], c12, s);
                P[tri<3>(i, j)] = (i == j) ? s + q[i] * dt : s;
            }
        bool applied = (type == kGps || type == kImu);
        if (gated && applied) applied = gate.open(P, live, thr);
        bool ok = true;
        if (applied) {
            if (type == kGps) {
                if (pva) {
                    T zb[NL][1];
#pragma unroll
                    for (int v = 0; v < NL; ++v) zb[v][0] = va;
                    const T R[1] = {Rgps};
                    if constexpr (SCORE) {
                        Innov<T, 1> inn;
                        ok = sel_update_nv<3, 1, true, T, kRefNewton, true, NL, kRefJoseph<T>, kRefGainR, true>(
                            x, P, zb, R, &inn);
                        sc->add(0, inn);
                    } else {
                        ok = sel_update_nv<3, 1, true, T, kRefNewton, true, NL, kRefJoseph<T>, kRefGainR>(x, P, zb, R);
                    }
                }
                if constexpr (SCORE) sc->ngps += 1;
            } else {
                T zb[NL][3];
#pragma unroll
                for (int v = 0; v < NL; ++v) {
                    const T V = fmaT(vb, dt, x[v][1]);
                    const T X = fmaT(V, dt, x[v][0]);
                    zb[v][0] = pva ? X : va;
                    zb[v][1] = pva ? V : vb;
                    zb[v][2] = pva ? vb : T(0);
                }
                if constexpr (SCORE) {
                    Innov<T, 3> inn;
                    ok = sel_update_nv<3, 3, true, T, kRefNewton, true, NL, kRefJoseph<T>, kRefGainR, true>(
                        x, P, zb, Rimu, &inn);
                    sc->add(1, inn);
                } else {
                    ok = sel_update_nv<3, 3, true, T, kRefNewton, true, NL, kRefJoseph<T>, kRefGainR>(x, P, zb, Rimu);
                }
                if (!pva) {  // reset the inert state
#pragma unroll
                    for (int v = 0; v < NL; ++v) x[v][2] = T(0);
                    P[5] = T(1);
                }
            }
        }
        if (group_any(!ok)) {
            st = kNotSpd;
#pragma unroll
            for (int v = 0; v < NL; ++v)
#pragma unroll
                for (int k = 0; k < 3; ++k) x[v][k] = quiet_nan<T>();
#pragma unroll
            for (int k = 0; k < 6; ++k) P[k] = quiet_nan<T>();
        }
        return applied;
    }
};

// The input ring of the chain-layout kernels: event t's inputs are loaded D - 1 events ahead
// through a fully unrolled ring of named buffers (static indices, no loop-carried copies).
// load(t, in) is called for t up to n + D - 2 and clamps past-the-end events itself (they re-read
// a last event); the prologue's loads are drained once, so no in-loop wait targets them (vmcnt
// counts in order: the step's wait for its own buffer then leaves the D - 1 younger loads in
// flight).  Each depth adds a copy of the event body (48 KB of code at 8).  Depths 2, 3, 4 and 8
// were A/B-measured on config 1 (one filter, per-filter layout) without a resolvable difference: a
// single wave's launch time varies +-10% from launch to launch
// (profiles/r01_ab/chain_depth_inproc.json), so that default stays at 2.  Stream mode gathers
// each filter's events from its own part of the stream (a cache line per 1.8 events, lines differ
// per filter), so its loads see HBM latency: a deeper ring.
template <int D, typename T, class In = ChainIn<T>, class Load, class Step>
__device__ __forceinline__ void ring_run(int n, Load&& load, Step&& step) {
    if (n <= 0) return;
    In buf[D];
#pragma unroll
    for (int j = 0; j < D - 1; ++j) load(j, buf[j]);
    __builtin_amdgcn_s_waitcnt(0);
    int t = 0;
    for (; t + D <= n; t += D) {
#pragma unroll
        for (int j = 0; j < D; ++j) {
            load(t + j + D - 1, buf[(j + D - 1) % D]);
            step(t + j, buf[j]);
        }
    }
#pragma unroll
    for (int j = 0; j < D - 1; ++j)
        if (t + j < n) step(t + j, buf[j]);
}

}  // namespace

}  // namespace kfmi

// The sweep-layout kernels of the reference models, 8 lanes per filter and one wave per workgroup
// (the lane is kf_ref_chainlane.h's): ref_sweep_kernel (kf_run_sweep, kf_run_sweep_params,
// kf_run_sweep_scores: launch_ref_sweep; kf_run_tails: launch_ref_tails) and the RTS smoother over
// a sweep's record, ref_smooth_kernel (kf_smooth_sweep: launch_ref_smooth; with the EM statistics,
// kf_smooth_sweep_em: launch_ref_smooth_em).
#include "kf_ref_chainlane.h"

namespace kfmi {
namespace {

// ------------------------------------------------------------------------------------
// Threshold sweep (kf_run_sweep): ONE event stream [T] run by B gated filters that differ only in
// their adaptive threshold (kf_workers.py:959-1058; the experiment loop's r_value draw,
// :2298-2317) and their start state.  The chain kernel's layout, 8 lanes per filter and lane c on
// axis chain c, so a wave carries 8 thresholds; every group reads the same stream entries (byte
// range descriptors as in stream mode: the 8 groups' loads hit one cache line), and the event's
// type and dt are wave-uniform.  Each event is ChainLane::event, gated by the group's own
// threshold.  The groups of a wave disagree about `applied`, so the wave pays the update whenever
// one of its groups applies it: a sweep costs about what its most-updating threshold costs.  Records in kf_run_events' layouts ([T][W][B], [T][B]), an
// update count per filter, and the handle-layout state every ckpt_every events.
//
// TAILS (kf_run_tails): the same groups as ragged tails of the one stream.  Group f gathers its
// start state itself (row tails[f].src_row, column src_col of src_x / src_P, or its own handle
// column), runs the events [lo, hi) of the stream and writes its end state to handle column f; no
// records, no checkpoints.  The event's type and dt are the group's own, so the NONE / GPS / IMU
// branches diverge between groups (a group is active or inactive as a whole: its DPP reductions
// stay legal).  The wave runs to its longest tail with the finished groups predicated off, and
// the input ring clamps per group to the tail's own last event; an empty tail loads nothing.
//
// PARAMS (kf_run_sweep_params): the groups differ in their noise constants as well.  Lane set-up
// fills the lane's q / Rimu / Rgps from column f of a.consts (ChainLane's table constructor)
// instead of the literals or the handle's scalars, once, beside the threshold and before the
// ring's prologue, whose drain covers those loads too; a.thresholds may be null (every group
// -inf).  Everything after set-up is the sweep's: the ring, ChainLane::event, the records.
//
// SCORE (kf_run_sweep_scores; PARAMS only): the run ranked where it runs.  Each lane keeps a
// ScoreAcc for its own chain, fed in event order: an applied update adds the NIS terms and the
// pivots that sel_update_nv's INNOV hands out of the update itself, and after every event a pva
// lane adds its axis' squared distance to the track row, which came through the ring with the
// event's inputs (NP more loads per event: the compiler counts the ring's in-loop vmcnt waits per
// instantiation, and the prologue's drain is a full one).  No atomics: after the last event one
// group_sum per row, and lane 0 stores the eight rows.  The filter's own arithmetic, records and
// checkpoints are the PARAMS kernel's.
// ------------------------------------------------------------------------------------
#ifndef KF_SWEEP_DEPTH
#define KF_SWEEP_DEPTH 4
#endif
constexpr int kSweepDepth = KF_SWEEP_DEPTH;  // input ring of ref_sweep_kernel
constexpr int kSweepBlock = 64;              // one wave (8 thresholds) per workgroup: waves spread over the CUs

// where group f's lanes take their constants from: the handle's, or PARAMS: column f of the table
template <bool PARAMS>
__device__ __forceinline__ auto sweep_consts(const SweepArgs& a, int64_t f) {
    if constexpr (PARAMS) return ConstsColumn{a.consts, a.B, f};
    else return a.kc;
}

template <typename T, class M, bool CUSTOM, bool TAILS = false, bool PARAMS = false, bool SCORE = false>
__global__ __launch_bounds__(kSweepBlock) void ref_sweep_kernel(const SweepArgs a) {
    static_assert(!PARAMS || (!TAILS && !CUSTOM), "per-filter constants: the plain sweep, in place of the handle's");
    static_assert(!SCORE || PARAMS, "scores: the parameter sweep's (track and scores share the tails' slots)");
    static_assert(consts_rows(M::N) == 2 * M::N + M::NP, "the table's rows: q, r_imu, r_gps");
    const int64_t g = static_cast<int64_t>(blockIdx.x) * kSweepBlock + threadIdx.x;
    const int64_t f = g / kGroup;
    // TAILS: the group's tail, and the wave's longest (every lane of the wave takes part in the
    // reduction, the groups past B with length 0, before those leave)
    TailSpec tl{0, 0, -1, 0};
    int len = 0, wave_len = 0;
    if constexpr (TAILS) {
        if (f < a.B) {
            tl = a.tails[f];
            len = tl.hi - tl.lo;
        }
        wave_len = len;
#pragma unroll
        for (int sh = kGroup; sh < 64; sh <<= 1) wave_len = max(wave_len, __shfl_xor(wave_len, sh, 64));
        wave_len = wave_uniform(wave_len);
    }
    if (f >= a.B) return;  // whole groups leave together
    const ChainLane<T, M, CUSTOM> L(static_cast<int>(g % kGroup), sweep_consts<PARAMS>(a, f));
    const int c = L.c;
    const bool live = L.live;
    const auto& xi = L.xi;
    const auto& pr = L.pr;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(a.B) * uint32_t(sizeof(T));
    uint32_t vx[3], vp[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) vx[k] = xi[k] >= 0 ? uint32_t(xi[k]) * rb + off : kDropOffset;
#pragma unroll
    for (int k = 0; k < 6; ++k) vp[k] = pr[k] >= 0 ? uint32_t(pr[k]) * rb + off : kDropOffset;
    const uint32_t v_tr = (xi[0] >= 0 && xi[0] < M::NTRAJ) ? uint32_t(xi[0]) * rb + off : kDropOffset;
    const uint32_t v_ld = c == 0 ? off : kDropOffset;
    const uint32_t v_up = c == 0 ? uint32_t(f) : kDropOffset;

    T x[1][3], P[6];
    if constexpr (TAILS) {
        // the group's own source column (64-bit addressing: row src_row of [R][rows][src_B]), or
        // its handle column; the rows a lane does not hold keep the handle load's 0 / 1
        const bool own = tl.src_row < 0;
        const int64_t sb = own ? a.B : a.src_B;
        const T* sx = own ? static_cast<const T*>(a.x) + f
                          : static_cast<const T*>(a.src_x) + int64_t(tl.src_row) * M::N * sb + tl.src_col;
        const T* sp = own ? static_cast<const T*>(a.P) + f
                          : static_cast<const T*>(a.src_P) + int64_t(tl.src_row) * M::NBLK * sb + tl.src_col;
#pragma unroll
        for (int k = 0; k < 3; ++k) x[0][k] = xi[k] >= 0 ? sx[int64_t(xi[k]) * sb] : T(0);
#pragma unroll
        for (int k = 0; k < 6; ++k) P[k] = pr[k] >= 0 ? sp[int64_t(pr[k]) * sb] : L.unit(k);
    } else {
        const auto rx = span_rsrc(a.x, 0, rb, M::N), rp = span_rsrc(a.P, 0, rb, M::NBLK);
#pragma unroll
        for (int k = 0; k < 3; ++k) x[0][k] = ldv(rx, vx[k], T(0));
#pragma unroll
        for (int k = 0; k < 6; ++k) P[k] = pr[k] >= 0 ? ldv(rp, vp[k], T(0)) : L.unit(k);
    }
    // a tail from a source column starts with status OK, as after kf_set_state
    int32_t st = (TAILS && tl.src_row >= 0) ? 0 : a.status[f];
    int32_t nup = 0;
    // the group's threshold; NaN never opens the gate (every comparison with it is false), and
    // -inf is "always update": the gate is not evaluated (a covariance that is not positive
    // definite has no log-det to compare, and the reference's slogdet still passes -inf there)
    const double thr_d = (PARAMS && !a.thresholds) ? -__builtin_inf() : a.thresholds[f];
    const T thr = T(thr_d);
    const bool always = thr_d == -__builtin_inf();
    GateBand<T> gate;
    gate.init(thr_d);
    const bool need_tr = !TAILS && a.traj != nullptr, need_ld = !TAILS && a.logdet != nullptr;
    const bool need_up = !TAILS && a.updated != nullptr;

    const uint32_t S = uint32_t(a.T);
    const auto r_et = bytes_rsrc(a.etype, S), r_dt = bytes_rsrc(a.dt, S * 8u);
    const auto r_pay = bytes_rsrc(a.payload, S * 9u * uint32_t(sizeof(T)));
    // stream event ue's inputs; dead = ~0u drops the loads (offset 2^32 - 1 lies past every byte
    // range, the 4 GiB payload's too)
    // SCORE: track row ue rides in the ring with the event's other inputs, the ring's last loads:
    // a pva lane loads the columns the model reads, its own first (a null track: a zero-length
    // range, loads nothing, scores nothing); the other lanes' loads are dropped (~0u lies past
    // every byte range, 24 T < 2^32)
    // (everything of SCORE sits under if constexpr or in a type that is empty without it: the
    // other instantiations must stay the instruction streams they were)
    using In = std::conditional_t<SCORE, ChainInScored<T>, ChainIn<T>>;
    struct NoScore {};
    std::conditional_t<SCORE, ScoreAcc, NoScore> sc;
    auto load = [&](uint32_t ue, uint32_t dead, In& in) {
        in.type = int(__builtin_amdgcn_raw_buffer_load_b8(r_et, ue | dead, 0, 0));
        in.dt = ldv(r_dt, (ue * 8u) | dead, 0.0);
        in.va = ldv(r_pay, ((ue * 9u + uint32_t(L.ia)) * uint32_t(sizeof(T))) | dead, T(0));
        in.vb = ldv(r_pay, ((ue * 9u + uint32_t(L.ib)) * uint32_t(sizeof(T))) | dead, T(0));
        if constexpr (SCORE) {
            const auto r_trk = bytes_rsrc(a.track, S * 24u);
            const uint32_t m_trk = L.pva ? 0u : ~0u;
#pragma unroll
            for (int k = 0; k < 3; ++k)
                in.track[k] = k < M::NP ? ldv(r_trk, (ue * 24u + uint32_t((L.ca + k) % M::NP) * 8u) | m_trk | dead, 0.0)
                                        : 0.0;
        }
    };
    int ck_left = TAILS ? 0 : a.ckpt_every;  // events until the next checkpoint (wave-uniform)
    int ck_row = 0;
    auto step = [&](int t, const In& in) {
        // every lane of the wave loaded the same type and dt: scalars (TAILS: the group's own)
        const int type = TAILS ? in.type : wave_uniform(in.type);
        bool applied;
        if constexpr (SCORE) {
            applied = L.template event<1, true>(type, T(in.dt), in.va, in.vb, !always, gate, thr, x, P, st, &sc);
            // the event's position against its track row, whatever its type: scored when every
            // column the model reads is a number (a NaN in any of them: no reference here)
            if (a.track != nullptr) {  // wave-uniform
                const bool have = !(in.track[0] != in.track[0] || in.track[1] != in.track[1] ||
                                    in.track[2] != in.track[2]);
                const double e = have ? double(x[0][0]) - in.track[0] : 0.0;
                sc.npos += have ? 1 : 0;
                sc.sse = __builtin_fma(e, e, sc.sse);
            }
        } else {
            applied = L.event(type, T(in.dt), in.va, in.vb, !always, gate, thr, x, P, st);
        }
        nup += applied ? 1 : 0;
        // absent records: skipped by wave-uniform branches
        if (need_tr) stv(span_rsrc(a.traj, int64_t(t) * M::NTRAJ, rb, M::NTRAJ), v_tr, x[0][0]);
        if (need_ld) {
            const T ld = group_sum(live ? chain_log_det(P) : T(0));
            st = (ld == ld) ? st : kNotSpd;
            stv(span_rsrc(a.logdet, t, rb, 1), v_ld, ld);
        }
        if (need_up)
            __builtin_amdgcn_raw_buffer_store_b8(applied ? uint8_t(1) : uint8_t(0),
                                                 span_rsrc(a.updated, t, uint32_t(a.B), 1), v_up, 0, 0);
        if (ck_left > 0 && --ck_left == 0) {  // checkpoint row ck_row: the filter after this event
            ck_left = a.ckpt_every;
            const auto cx = span_rsrc(a.ckpt_x, int64_t(ck_row) * M::N, rb, M::N);
            const auto cp = span_rsrc(a.ckpt_P, int64_t(ck_row) * M::NBLK, rb, M::NBLK);
#pragma unroll
            for (int k = 0; k < 3; ++k) stv(cx, vx[k], x[0][k]);
#pragma unroll
            for (int k = 0; k < 6; ++k) stv(cp, vp[k], P[k]);
            ++ck_row;
        }
    };

    if constexpr (TAILS) {
        // the ring over the wave's longest tail (finite, wave-uniform, known before the loop): step s
        // is the group's event lo + s, its loads clamped to the tail's own last event (so never past
        // T - 1); a group past its tail is predicated off, and an empty tail loads nothing
        const uint32_t dead = len > 0 ? 0u : ~0u;
        ring_run<kSweepDepth, T>(
            wave_len, [&](int s, ChainIn<T>& in) { load(uint32_t(tl.lo + (s < len ? s : len - 1)), dead, in); },
            [&](int s, const ChainIn<T>& in) {
                if (s < len) step(s, in);
            });
    } else {
        const int T_ = a.T;
        ring_run<kSweepDepth, T, In>(T_, [&](int t, In& in) { load(uint32_t(t < T_ ? t : T_ - 1), 0u, in); }, step);
    }
    {
        const auto rx = span_rsrc(a.x, 0, rb, M::N), rp = span_rsrc(a.P, 0, rb, M::NBLK);
#pragma unroll
        for (int k = 0; k < 3; ++k) stv(rx, vx[k], x[0][k]);
#pragma unroll
        for (int k = 0; k < 6; ++k) stv(rp, vp[k], P[k]);
    }
    {
        const auto rs = span_rsrc(a.status, 0, uint32_t(a.B) * 4u, 1);
        __builtin_amdgcn_raw_buffer_store_b32(uint32_t(st), rs, c == 0 ? uint32_t(f) * 4u : kDropOffset, 0, 0);
        if (a.n_updated) {
            const auto rn = span_rsrc(a.n_updated, 0, uint32_t(a.B) * 4u, 1);
            __builtin_amdgcn_raw_buffer_store_b32(uint32_t(nup), rn, c == 0 ? uint32_t(f) * 4u : kDropOffset, 0, 0);
        }
    }
    if constexpr (SCORE) {
        // the eight rows of column f: each float row one group_sum of the chains' own sums (a GPS
        // row: the pva chains'), the logs taken here, once; NaN where the filter failed.  Lane 0
        // stores them (row r at r B 8 + f 8 of one span; 64 B < 2^31 by the state span's limit).
        const bool pva = L.pva;
        const double nan = quiet_nan<double>();
        const bool bad = st != 0;
        double row[kScoreRows];
        const int32_t nimu = nup - sc.ngps;  // every applied update is a fix or an IMU event
        row[kScoreGpsN] = double(sc.ngps);
        row[kScoreGpsNis] = group_sum(pva ? sc.nis[0] : 0.0);
        row[kScoreGpsLogdetS] = group_sum(pva ? log_mant(sc.ldm[0], sc.lde[0]) : 0.0);
        row[kScoreImuN] = double(nimu);
        row[kScoreImuNis] = group_sum(live ? sc.nis[1] : 0.0);
        // an aw chain's S is 2 x 2: its inert third pivot, exactly 2 every update, out of the exponent
        row[kScoreImuLogdetS] = group_sum(live ? log_mant(sc.ldm[1], sc.lde[1] - (pva ? 0 : nimu)) : 0.0);
        row[kScorePosN] = double(sc.npos);
        row[kScorePosSse] = group_sum(pva ? sc.sse : 0.0);
        const auto rs = span_rsrc(a.scores, 0, uint32_t(a.B) * 8u, kScoreRows);
#pragma unroll
        for (int r = 0; r < kScoreRows; ++r) {
            const bool count = r == kScoreGpsN || r == kScoreImuN || r == kScorePosN;
            stv(rs, c == 0 ? (uint32_t(r) * uint32_t(a.B) + uint32_t(f)) * 8u : kDropOffset,
                bad && !count ? nan : row[r]);
        }
    }
}

// ------------------------------------------------------------------------------------
// Fixed-interval (Rauch-Tung-Striebel) smoother over a sweep's filtered record (kf_smooth_sweep):
// the backward pass over ckpt_x / ckpt_P of a sweep with ckpt_every = 1, in the sweep's layout (8
// lanes per filter, lane c on axis chain c, one wave per workgroup).  P is block-diagonal over the
// chains and F acts within a chain, so the smoother gain is block-diagonal too: each lane smooths
// its own 3 x 3 block and holds the smoothed (x, P) of event t + 1 in registers, 3 + 6 values.
// Row T - 1 is the filtered row.  For t = T - 2 .. 0, with (x_f, P_f) the filtered row t:
//   etype[t + 1] == NONE: the forward step changed nothing, row t is row t + 1 (no arithmetic);
//   otherwise  x_p = F x_f, P_p = F P_f F^T + Q dt[t + 1]   (ChainLane::predict, so P_p is the
//                                                           forward run's own P_pred bit for bit)
//              C = (P_f F^T) P_p^-1                         (in-lane LDL^T of P_p; its three pivots'
//                                                           reciprocals are IEEE divisions, see there)
//              x_s[t] = x_f + C (x_s[t + 1] - x_p)
//              P_s[t] = P_f + C (P_s[t + 1] - P_p) C^T      (once per packed entry i <= j)
// whatever the event at t + 1 was: its update is already in x_s[t + 1].  A lane without a chain
// runs the same code on the unit block; an aw lane's inert third state stays (0, 1).
// The inputs come backwards through ring_run (step s is t = T - 2 - s): etype and dt of t + 1 by
// byte-range descriptors, the lane's 3 + 6 values of row t by a span descriptor with a 64-bit base
// per event.  A row is loaded kSmoothDepth - 1 steps before the step that may overwrite it, so
// sm_x == filt_x and sm_P == filt_P are legal.  No atomics, no LDS, no workspace.
// A non-positive pivot of P_p or a NaN in a loaded row poisons the filter's group from that t down
// to 0 (NaN rows, KF_ENOTSPD in sm_status); the rows above it are already stored.
//
// EM (kf_smooth_sweep_em; PARAMS too, the argument block is then SmoothEmArgs): the sufficient
// statistics of the diagonal Q, R_imu and R_gps, everything under `if constexpr` or in a type that
// is empty without it, so the other instantiations stay the instruction streams they were
// (profiles/sweep_em/isa_compare.log).  All of it lane-local and summed in backward step order, in
// double: the lane that smooths a chain holds that chain's Q rows and R rows (J below is
// block-diagonal as C is), so no group_sum, no atomics, no LDS, no workspace.
//   the transition into event t + 1 (counted when its type is not NONE and d = dt[t + 1] != 0):
//     J = Q d P_p^-1 by the step's own L, D and reciprocals (row i: one more right-hand side),
//     E[w | all] = J (x_s[t + 1] - x_p), Var[w | all] = Q d + J (P_s[t + 1] - P_p) J^T, and state i
//     adds (E[w]_i^2 + Var[w]_ii) / d.  No lag-one covariance, no row t - 1.
//   the applied update of event t + 1 (updated[t + 1][f] != 0; the byte and the lane's two payload
//     values of that event ride in the ring): z rebuilt as ChainLane::event built it (GPS: the
//     payload; IMU: event's own X / V / zb lines on x_p, restated here: sharing them would move
//     event's instruction stream), then (z_i - x_s[t + 1]_i)^2 + P_s[t + 1]_ii per measured state.
//   Event 0 starts the interval: neither its transition nor its update is counted.
// The counts sit on lane 0 of the group; every lane stores its own rows once, after the last step,
// NaN where the filter was poisoned (the counts stay).
// ------------------------------------------------------------------------------------
#ifndef KF_SMOOTH_DEPTH
#define KF_SMOOTH_DEPTH KF_SWEEP_DEPTH
#endif
constexpr int kSmoothDepth = KF_SMOOTH_DEPTH;  // input ring of ref_smooth_kernel

// One backward step's inputs for one lane: the event after the row, and the lane's part of the row
template <typename T>
struct SmoothIn {
    int type;
    double dt;
    T x[3], P[6];
};
// EM: the lane's two payload values of that event and the filter's `updated` byte ride along
template <typename T>
struct SmoothInEm : SmoothIn<T> {
    T va, vb;
    int up;
};
// EM: one lane's accumulators (kf_smooth_sweep_em)
struct RefEmAcc {
    int32_t ntrans = 0, ngps = 0, nimu = 0;
    double q[3] = {0.0, 0.0, 0.0};
    double rimu[3] = {0.0, 0.0, 0.0};
    double rgps = 0.0;
};

__device__ __forceinline__ const SmoothArgs& smooth_args(const SmoothArgs& a) { return a; }
__device__ __forceinline__ const SmoothArgs& smooth_args(const SmoothEmArgs& a) { return a.smooth; }

// EM: column f of the table or, without one, the handle's constants: one pair of instantiations
// serves every handle (ChainLane's ConstsOrHandle constructor)
template <bool PARAMS, bool EM = false>
__device__ __forceinline__ auto smooth_consts(const SmoothArgs& a, int64_t f) {
    if constexpr (EM) return ConstsOrHandle{{a.consts, a.B, f}, a.kc};
    else if constexpr (PARAMS) return ConstsColumn{a.consts, a.B, f};
    else return a.kc;
}

template <typename T, class M, bool CUSTOM, bool PARAMS = false, bool EM = false, int DEPTH = kSmoothDepth,
          typename A = SmoothArgs>
__global__ __launch_bounds__(kSweepBlock) void ref_smooth_kernel(const A ka) {
    static_assert(!PARAMS || !CUSTOM, "per-filter constants in place of the handle's");
    static_assert(PARAMS || !EM, "EM takes its constants as PARAMS does (or, without a table, the handle's)");
    static_assert(std::is_same_v<A, std::conditional_t<EM, SmoothEmArgs, SmoothArgs>>, "EM: its own argument block");
    const SmoothArgs& a = smooth_args(ka);
    const int64_t g = static_cast<int64_t>(blockIdx.x) * kSweepBlock + threadIdx.x;
    const int64_t f = g / kGroup;
    if (f >= a.B) return;  // whole groups leave together
    const ChainLane<T, M, CUSTOM> L(static_cast<int>(g % kGroup), smooth_consts<PARAMS, EM>(a, f));
    const int c = L.c;
    const bool live = L.live;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(a.B) * uint32_t(sizeof(T));
    uint32_t vx[3], vp[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) vx[k] = L.xi[k] >= 0 ? uint32_t(L.xi[k]) * rb + off : kDropOffset;
#pragma unroll
    for (int k = 0; k < 6; ++k) vp[k] = L.pr[k] >= 0 ? uint32_t(L.pr[k]) * rb + off : kDropOffset;
    const uint32_t v_tr = (L.xi[0] >= 0 && L.xi[0] < M::NTRAJ) ? uint32_t(L.xi[0]) * rb + off : kDropOffset;
    const uint32_t v_ld = c == 0 ? off : kDropOffset;
    const bool need_x = a.sm_x != nullptr, need_P = a.sm_P != nullptr;
    const bool need_tr = a.sm_traj != nullptr, need_ld = a.sm_logdet != nullptr;

    const int T_ = a.T;
    const uint32_t S = uint32_t(T_);
    const auto r_et = bytes_rsrc(a.etype, S), r_dt = bytes_rsrc(a.dt, S * 8u);
    // row t of the filtered record: the lane's states and block rows (the rows it does not hold
    // are dropped loads, 0, and the identity's entries)
    auto load_row = [&](int t, T (&x)[3], T (&P)[6]) {
        const auto rx = span_rsrc(a.filt_x, int64_t(t) * M::N, rb, M::N);
        const auto rp = span_rsrc(a.filt_P, int64_t(t) * M::NBLK, rb, M::NBLK);
#pragma unroll
        for (int k = 0; k < 3; ++k) x[k] = ldv(rx, vx[k], T(0));
#pragma unroll
        for (int k = 0; k < 6; ++k) P[k] = L.pr[k] >= 0 ? ldv(rp, vp[k], T(0)) : L.unit(k);
    };
    auto is_nan_row = [&](const T (&x)[3], const T (&P)[6]) {
        bool nan = false;
#pragma unroll
        for (int k = 0; k < 3; ++k) nan = nan || x[k] != x[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) nan = nan || P[k] != P[k];
        return nan;
    };
    int32_t st = 0;
    T xs[1][3], Ps[6];  // the smoothed row t + 1
    auto poison = [&]() {
        st = kNotSpd;
#pragma unroll
        for (int k = 0; k < 3; ++k) xs[0][k] = quiet_nan<T>();
#pragma unroll
        for (int k = 0; k < 6; ++k) Ps[k] = quiet_nan<T>();
    };
    // absent outputs: skipped by wave-uniform branches
    auto store_row = [&](int t) {
        if (need_x) {
            const auto rx = span_rsrc(a.sm_x, int64_t(t) * M::N, rb, M::N);
#pragma unroll
            for (int k = 0; k < 3; ++k) stv(rx, vx[k], xs[0][k]);
        }
        if (need_P) {
            const auto rp = span_rsrc(a.sm_P, int64_t(t) * M::NBLK, rb, M::NBLK);
#pragma unroll
            for (int k = 0; k < 6; ++k) stv(rp, vp[k], Ps[k]);
        }
        if (need_tr) stv(span_rsrc(a.sm_traj, int64_t(t) * M::NTRAJ, rb, M::NTRAJ), v_tr, xs[0][0]);
        if (need_ld) {
            const T ld = group_sum(live ? chain_log_det(Ps) : T(0));
            stv(span_rsrc(a.sm_logdet, t, rb, 1), v_ld, ld);
        }
    };

    // row T - 1: the filtered row itself
    load_row(T_ - 1, xs[0], Ps);
    __builtin_amdgcn_s_waitcnt(0);
    if (group_any(live && is_nan_row(xs[0], Ps))) poison();
    store_row(T_ - 1);

    const int n = T_ - 1;  // backward steps; step s is row t = T - 2 - s (past the end: row 0 again)
    using In = std::conditional_t<EM, SmoothInEm<T>, SmoothIn<T>>;
    struct NoEm {};
    std::conditional_t<EM, RefEmAcc, NoEm> em;
    auto load = [&](int s, In& in) {
        const int t = T_ - 2 - (s < n ? s : n - 1);
        in.type = int(__builtin_amdgcn_raw_buffer_load_b8(r_et, uint32_t(t + 1), 0, 0));
        in.dt = ldv(r_dt, uint32_t(t + 1) * 8u, 0.0);
        load_row(t, in.x, in.P);
        if constexpr (EM) {
            // event t + 1's measurement, the ring's last loads: the lane's two payload columns
            // (ref_sweep_kernel's) by byte range, and the filter's byte of row t + 1 of `updated`, a
            // [B] span from a 64-bit base per event (null streams: zero-length ranges, 0)
            const auto r_pay = bytes_rsrc(ka.payload, S * 9u * uint32_t(sizeof(T)));
            in.va = ldv(r_pay, (uint32_t(t + 1) * 9u + uint32_t(L.ia)) * uint32_t(sizeof(T)), T(0));
            in.vb = ldv(r_pay, (uint32_t(t + 1) * 9u + uint32_t(L.ib)) * uint32_t(sizeof(T)), T(0));
            in.up = int(__builtin_amdgcn_raw_buffer_load_b8(span_rsrc(ka.updated, t + 1, uint32_t(a.B), 1), uint32_t(f), 0, 0));
        }
    };
    auto step = [&](int s, const In& in) {
        const int t = T_ - 2 - s;
        const int type = wave_uniform(in.type);  // every lane loaded the same type and dt
        bool bad = is_nan_row(in.x, in.P);
        if (type != 255) {
            const T dt = T(in.dt);
            T xp[1][3] = {{in.x[0], in.x[1], in.x[2]}};
            T Pp[6], FP[3][3];
#pragma unroll
            for (int k = 0; k < 6; ++k) Pp[k] = in.P[k];
            L.template predict<1>(dt, xp, Pp, FP);
            // P_p = L D L^T (unit lower L).  The pivots' reciprocals are IEEE divisions, not the
            // updates' rcp_nr<kRefNewton>: P_f - C P_p C^T cancels (between applied updates P_s is
            // orders of magnitude below P_f) and a relative error e of a pivot's reciprocal is the
            // same wrong P_p^-1 in all three rows of C, so it reaches P_s as e P_f.  Measured against
            // the longdouble truth at T = 300, in units of the plain float64 NumPy smoother's own
            // error, budget 8 (profiles/rts_smoother/reciprocal_forms.log): with rcp_nr<kRefNewton>
            // (2^-46) log det P_s reached 8.4 at the first case that failed; with a step of
            // iterative refinement of C on top, P_s 8.9 and log det 36 (the residual rounds at
            // eps |C| |P_p|); with divisions at most 2.0 and 4.8.  Three divisions a step
            const T d0 = Pp[0];
            const T i0 = T(1) / d0;
            const T l10 = Pp[1] * i0, l20 = Pp[2] * i0;
            const T v0 = l10 * d0;
            const T d1 = fmaT(-l10, v0, Pp[3]);
            const T i1 = T(1) / d1;
            const T l21 = fmaT(-l20, v0, Pp[4]) * i1;
            const T d2 = fmaT(-l21, l21 * d1, fmaT(-l20, l20 * d0, Pp[5]));
            const T i2 = T(1) / d2;
            bad = bad || !(d0 > T(0) && d1 > T(0) && d2 > T(0));
            // C = (P_f F^T) P_p^-1, row i: P_p c = row i of (F P_f)^T = column i of F P_f
            T C[3][3];
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                const T w0 = FP[0][i];
                const T w1 = fmaT(-l10, w0, FP[1][i]);
                const T w2 = fmaT(-l21, w1, fmaT(-l20, w0, FP[2][i]));
                const T c2 = w2 * i2;
                const T c1 = fmaT(-l21, c2, w1 * i1);
                const T c0 = fmaT(-l20, c2, fmaT(-l10, c1, w0 * i0));
                C[i][0] = c0, C[i][1] = c1, C[i][2] = c2;
            }
            T dx[3], D[6];
#pragma unroll
            for (int k = 0; k < 3; ++k) dx[k] = xs[0][k] - xp[0][k];
#pragma unroll
            for (int k = 0; k < 6; ++k) D[k] = Ps[k] - Pp[k];
            if constexpr (EM) {
                // the transition into event t + 1; one of no duration carries no noise and is not
                // counted (wave-uniform).  Row i of J: P_p j = q_i d e_i
                const bool count = in.dt != 0.0;
                const T inv_d = T(1) / (count ? dt : T(1));
                em.ntrans += count ? 1 : 0;
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const T qd = L.q[i] * dt;
                    const T w0 = i == 0 ? qd : T(0);
                    const T w1 = i == 1 ? qd : fmaT(-l10, w0, T(0));
                    const T w2 = i == 2 ? qd : fmaT(-l21, w1, fmaT(-l20, w0, T(0)));
                    const T j2 = w2 * i2;
                    const T j1 = fmaT(-l21, j2, w1 * i1);
                    const T j0 = fmaT(-l20, j2, fmaT(-l10, j1, w0 * i0));
                    const T ew = fmaT(j2, dx[2], fmaT(j1, dx[1], j0 * dx[0]));
                    const T jd0 = fmaT(j2, D[tri<3>(2, 0)], fmaT(j1, D[tri<3>(1, 0)], j0 * D[tri<3>(0, 0)]));
                    const T jd1 = fmaT(j2, D[tri<3>(2, 1)], fmaT(j1, D[tri<3>(1, 1)], j0 * D[tri<3>(0, 1)]));
                    const T jd2 = fmaT(j2, D[tri<3>(2, 2)], fmaT(j1, D[tri<3>(1, 2)], j0 * D[tri<3>(0, 2)]));
                    const T var = fmaT(jd2, j2, fmaT(jd1, j1, fmaT(jd0, j0, qd)));
                    em.q[i] += count ? double(fmaT(ew, ew, var) * inv_d) : 0.0;
                }
                // the applied update of event t + 1 against the smoothed row t + 1, still in xs / Ps:
                // z as the forward step built it from x_p (ChainLane::event's lines)
                if (in.up != 0 && (type == kGps || type == kImu)) {
                    if (type == kGps) {
                        const T e = in.va - xs[0][0];
                        em.rgps += double(fmaT(e, e, Ps[0]));
                        em.ngps += 1;
                    } else {
                        const T V = fmaT(in.vb, dt, xp[0][1]);
                        const T X = fmaT(V, dt, xp[0][0]);
                        const T z[3] = {L.pva ? X : in.va, L.pva ? V : in.vb, L.pva ? in.vb : T(0)};
#pragma unroll
                        for (int k = 0; k < 3; ++k) {
                            const T e = z[k] - xs[0][k];
                            em.rimu[k] += double(fmaT(e, e, Ps[tri<3>(k, k)]));
                        }
                        em.nimu += 1;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
                xs[0][i] = fmaT(C[i][2], dx[2], fmaT(C[i][1], dx[1], fmaT(C[i][0], dx[0], in.x[i])));
            T CD[3][3];  // C D
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    CD[i][j] = fmaT(C[i][2], D[tri<3>(2, j)], fmaT(C[i][1], D[tri<3>(1, j)], C[i][0] * D[tri<3>(0, j)]));
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = i; j < 3; ++j)
                    Ps[tri<3>(i, j)] =
                        fmaT(CD[i][2], C[j][2], fmaT(CD[i][1], C[j][1], fmaT(CD[i][0], C[j][0], in.P[tri<3>(i, j)])));
            if (!L.pva) {  // the inert state, as after the forward run's updates
                xs[0][2] = T(0);
                Ps[2] = Ps[4] = T(0);
                Ps[5] = T(1);
            }
        }
        if (group_any(live && bad) || st != 0) poison();
        store_row(t);
    };
    ring_run<DEPTH, T, In>(n, load, step);
    if (a.sm_status) {
        const auto rs = span_rsrc(a.sm_status, 0, uint32_t(a.B) * 4u, 1);
        __builtin_amdgcn_raw_buffer_store_b32(uint32_t(st), rs, c == 0 ? uint32_t(f) * 4u : kDropOffset, 0, 0);
    }
    if constexpr (EM) {
        // rows KF_REF_EM_* of column f, one span (row r at (r B + f) 8; ROWS B 8 < 2^31, checked by
        // the caller): lane 0 the counts, every lane its states' Q and R_imu rows, a pva lane its
        // axis' R_gps row; a filter that failed keeps its counts only.  A null table: nothing stored
        if (ka.em != nullptr) {  // wave-uniform
            constexpr int kRows = ref_em_rows(M::N);
            const auto re = span_rsrc(ka.em, 0, uint32_t(a.B) * 8u, kRows);
            const uint32_t rb8 = uint32_t(a.B) * 8u, off8 = uint32_t(f) * 8u;
            const double nanv = quiet_nan<double>();
            const bool good = st == 0;
            auto at = [&](bool have, int row) { return have ? uint32_t(row) * rb8 + off8 : kDropOffset; };
            stv(re, at(c == 0, kRefEmNTrans), double(em.ntrans));
            stv(re, at(c == 0, 1 + M::N), double(em.nimu));
            stv(re, at(c == 0, 2 + 2 * M::N), double(em.ngps));
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                stv(re, at(L.xi[k] >= 0, kRefEmQ + L.xi[k]), good ? em.q[k] : nanv);
                stv(re, at(L.xi[k] >= 0, 2 + M::N + L.xi[k]), good ? em.rimu[k] : nanv);
            }
            stv(re, at(L.pva, 3 + 2 * M::N + L.ca), good ? em.rgps : nanv);
        }
    }
}
}  // namespace

hipError_t launch_ref_tails(int model, bool f64, const SweepArgs& a, hipStream_t stream) {
    if (a.B <= 0 || a.T < 0 || !a.tails || (model != 15 && model != 8)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.B * kGroup + kSweepBlock - 1) / kSweepBlock));
    KF_REF_DISPATCH(model, f64, a.kc, ref_sweep_kernel<T, M, CUSTOM, true><<<grid, kSweepBlock, 0, stream>>>(a));
    return hipGetLastError();
}

hipError_t launch_ref_sweep(int model, bool f64, const SweepArgs& a, hipStream_t stream, bool scored) {
    if (a.B <= 0 || a.T <= 0 || (model != 15 && model != 8) || (!a.thresholds && !a.consts)) return hipErrorInvalidValue;
    if (scored && (!a.consts || !a.scores)) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.B * kGroup + kSweepBlock - 1) / kSweepBlock));
    if (a.consts)
        KF_BOOL_DISPATCH(scored, SCORE, KF_MODEL_DISPATCH(model, f64,
            ref_sweep_kernel<T, M, false, false, true, SCORE><<<grid, kSweepBlock, 0, stream>>>(a)));
    else
        KF_REF_DISPATCH(model, f64, a.kc, ref_sweep_kernel<T, M, CUSTOM><<<grid, kSweepBlock, 0, stream>>>(a));
    return hipGetLastError();
}

hipError_t launch_ref_smooth(int model, const SmoothArgs& a, hipStream_t stream) {
    if (a.B <= 0 || a.T <= 0 || (model != 15 && model != 8) || !a.filt_x || !a.filt_P || !a.etype || !a.dt)
        return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.B * kGroup + kSweepBlock - 1) / kSweepBlock));
    if (a.consts)
        KF_MODEL_DISPATCH(model, true, if constexpr (sizeof(T) == 8)
                                           ref_smooth_kernel<T, M, false, true><<<grid, kSweepBlock, 0, stream>>>(a));
    else
        KF_REF_DISPATCH(model, true, a.kc, if constexpr (sizeof(T) == 8)
                                               ref_smooth_kernel<T, M, CUSTOM><<<grid, kSweepBlock, 0, stream>>>(a));
    return hipGetLastError();
}

// kf_smooth_sweep_em's instantiations: their input ring holds two payload values and the `updated`
// byte more per step.  Depths 2 and 4 were A/B-measured in one process on the 583k-event log at B = 64
// (profiles/sweep_em/sweep_em_timing.log): 655 / 585 ms (every output / table only) at 4 against
// 763 / 673 ms at 2, so 4, the smoother's own depth.  Running in place is legal at any depth: a
// step stores row t alone, after its own load of that row, and the rows still to be loaded lie below t
#ifndef KF_REF_EM_DEPTH
#define KF_REF_EM_DEPTH 4
#endif

hipError_t launch_ref_smooth_em(int model, const SmoothEmArgs& e, hipStream_t stream) {
    const SmoothArgs& a = e.smooth;
    if (a.B <= 0 || a.T <= 0 || (model != 15 && model != 8) || !a.filt_x || !a.filt_P || !a.etype || !a.dt ||
        !e.payload != !e.updated)
        return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.B * kGroup + kSweepBlock - 1) / kSweepBlock));
    if (model == 15)
        ref_smooth_kernel<double, M15, false, true, true, KF_REF_EM_DEPTH, SmoothEmArgs><<<grid, kSweepBlock, 0, stream>>>(e);
    else
        ref_smooth_kernel<double, M8, false, true, true, KF_REF_EM_DEPTH, SmoothEmArgs><<<grid, kSweepBlock, 0, stream>>>(e);
    return hipGetLastError();
}

}  // namespace kfmi

// The 8-lanes-per-filter chain kernels of the reference models (the lane is kf_ref_chainlane.h's):
// ref_chain_kernel, per-filter (kf_run_events' chain variant: launch_ref_events_chain) and in
// stream mode (kf_run_stream's chunks: launch_ref_stream), and the one-filter look-ahead kernel
// ref_chain_gated_kernel.  The sweep and the smoother are kf_ref_sweep.hip's.
#include "kf_ref_chainlane.h"

namespace kfmi {
namespace {

// ------------------------------------------------------------------------------------
// Chain-parallel variant of ref_events_kernel for few filters (a single drive log): one lane
// per axis chain, kGroup lanes per filter.  Without the adaptive gate the chains are
// independent filters sharing an event stream, so a filter's per-event instruction stream
// shrinks to one chain's; the log-determinant (and the gate) is the sum of the chains' logs
// over the lane group (xor shuffles).  Every lane runs a 3-state chain: an (att, rate) chain
// carries an inert third state (F couples nothing to it, Q = 0; its IMU row measures z = 0
// with R = 1 and is reset after each update), so pva and aw lanes execute the same code.
// The arithmetic per chain is the lane kernel's, operation for operation (the extra terms are
// exact zeros); only the logdet is summed per chain instead of multiplied then logged.
// ------------------------------------------------------------------------------------
#ifndef KF_CHAIN_DEPTH
#define KF_CHAIN_DEPTH 2
#endif
constexpr int kChainDepth = KF_CHAIN_DEPTH;  // input ring of ref_chain_kernel
#ifndef KF_STREAM_DEPTH
#define KF_STREAM_DEPTH 8
#endif
constexpr int kStreamDepth = KF_STREAM_DEPTH;  // its input ring in stream mode (kf_run_stream)
#ifndef KF_STREAM_VAR_DEPTH
#define KF_STREAM_VAR_DEPTH 4
#endif
// the map pass's ring (4 state variants per lane): shallower, so the lane fits 2 waves per SIMD
constexpr int kStreamVarDepth = KF_STREAM_VAR_DEPTH;
#ifndef KF_STREAM_LD_BATCH
#define KF_STREAM_LD_BATCH 1
#endif
// the map pass's log-det records: the group's determinant product per event, kept by lane
// (event mod 8) and logged every 8 events (one log per lane-8-events instead of per lane-event;
// the pass is bound by its instruction issue).  0: every lane logs its chain every event and the
// group sums the logs (the NV = 1 chain kernel's form)
constexpr bool kStreamLdBatch = KF_STREAM_LD_BATCH != 0;
#ifndef KF_STREAM_VAR_SPLIT
#define KF_STREAM_VAR_SPLIT 0
#endif
// the map pass's four state variants as two per lane over two 8-lane groups per chunk (variants
// 0, 1 and 2, 3): twice the waves, each lane's event a little shorter (the covariance work
// repeated in both groups).  Measured slower on config 1, 0.2196 vs 0.2045 ms per log in-process
// (profiles/r04_pmc/cfg1_diag/ab_split_sym_halves.log), so off; kept for A/B builds
constexpr bool kStreamVarSplit = KF_STREAM_VAR_SPLIT != 0;
// lanes per filter of ref_chain_kernel
template <int NV>
__host__ __device__ constexpr int chain_lanes() {
    return NV == 4 && kStreamVarSplit ? 2 * 8 : 8;
}

// non-negative doubles (and +NaN) order as their bit patterns: atomic max via uint64
__device__ __forceinline__ void atomic_max_pos(double* p, double v) {
    if (!(v >= 0.0)) v = __builtin_nan("");
    atomicMax(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v));
}

// NV > 1 (stream mode only): NV variants of each filter that differ only in their start state
// (kf_run_stream's map pass: a chunk from its guess and from the guess + delta on each chain
// component) share one lane.  The covariance recursion does not read the state, so P, S and K
// are computed once per event and every variant's state is updated with them (ChainLane::event's
// NL states through sel_update_nv).  Variant v's state is
// column v * B + f of a state bank of NV * B columns (the covariance: column f), and its
// trajectory records go to rows v * s_vstride.
// GATES (kf_run_events_gates, per-filter layout): each 8-lane group gates its filter by its own
// a.thresholds[f], its GateBand set from it as ref_sweep_kernel's groups do.
template <typename T, class M, bool STREAM, bool CUSTOM, int NV = 1, bool GATES = false>
__global__ __launch_bounds__(kBlock) void ref_chain_kernel(const RefArgs a) {
    static_assert(NV == 1 || STREAM, "state variants are a stream-mode feature");
    static_assert(!GATES || (!STREAM && NV == 1), "per-filter gates are a per-filter-layout feature");
    if (a.skip && *a.skip) return;  // the sequential fallback of a stream run that passed its checks
    constexpr int LPF = chain_lanes<NV>();         // lanes per filter
    constexpr int NL = LPF == 2 * kGroup ? 2 : NV;  // variants this lane holds
    const int64_t g = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t f = g / LPF;
    if (f >= a.B) return;  // whole groups leave together (LPF divides the wave)
    const ChainLane<T, M, CUSTOM> L(static_cast<int>(g % kGroup), a.kc);
    const int c = L.c;
    const bool pva = L.pva, live = L.live;
    const auto& xi = L.xi;
    const auto& pr = L.pr;
    const int vb = NL < NV ? int((g % LPF) / kGroup) * NL : 0;  // this lane's first variant
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(a.B) * uint32_t(sizeof(T));
    const uint32_t rbank = uint32_t(NV) * rb;  // row stride of the state / covariance bank
    const uint32_t rb8 = uint32_t(a.B) * 8u;
    const uint32_t off8 = uint32_t(f) * 8u;
    // this lane's state and block rows as voffsets into row spans
    uint32_t vx[3], vp[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) vx[k] = xi[k] >= 0 ? uint32_t(xi[k]) * rbank + off : kDropOffset;
#pragma unroll
    for (int k = 0; k < 6; ++k) vp[k] = pr[k] >= 0 ? uint32_t(pr[k]) * rbank + off : kDropOffset;
    const uint32_t v_tr = (xi[0] >= 0 && xi[0] < M::NTRAJ) ? uint32_t(xi[0]) * rb + off : kDropOffset;
    const uint32_t v_ld = c == 0 ? off : kDropOffset;
    const uint32_t v_a = uint32_t(L.ia) * rb + off, v_b = uint32_t(L.ib) * rb + off;

    T x[NL][3], P[6];
    T xs0[3];  // variant 0's start (the map pass's guess)
    {
        const auto rx = span_rsrc(a.x, 0, rbank, M::N), rp = span_rsrc(a.P, 0, rbank, M::NBLK);
#pragma unroll
        for (int v = 0; v < NL; ++v)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                x[v][k] = ldv(rx, vx[k] == kDropOffset ? kDropOffset : vx[k] + uint32_t(vb + v) * rb, T(0));
#pragma unroll
        for (int k = 0; k < 6; ++k) P[k] = pr[k] >= 0 ? ldv(rp, vp[k], T(0)) : L.unit(k);
        if constexpr (NL < NV) {
#pragma unroll
            for (int k = 0; k < 3; ++k) xs0[k] = ldv(rx, vx[k], T(0));
        } else {
#pragma unroll
            for (int k = 0; k < 3; ++k) xs0[k] = x[0][k];
        }
    }
    // the map pass's seam check reads the next chunk's start covariance: loaded here, before
    // any of this lane's stores (a later load would wait for all of them, vmcnt being in order)
    double wnx[6] = {0, 0, 0, 0, 0, 0};
    if constexpr (NV == 4) {
        if (live && a.s_maps && a.s_check && f + 1 < a.B) {
            const T* wn = static_cast<const T*>(a.s_wnext);
#pragma unroll
            for (int k = 0; k < 6; ++k)
                if (pr[k] >= 0) wnx[k] = double(wn[int64_t(pr[k]) * a.B + f + 1]);
        }
    }
    int32_t st = a.status[f];
    const bool need_ld = a.logdet != nullptr;
    FilterGate<T> fg{a.gate != 0, T(a.threshold)};  // the launch's gate, or GATES: the filter's own
    if constexpr (GATES) fg = gate_of<T>(a.thresholds, f);
    GateBand<T> gate;
    if (fg.on) gate.init(GATES ? a.thresholds[f] : a.threshold);
    constexpr bool kLdBatch = STREAM && NV == 4 && kStreamLdBatch;
    T bm = T(1);  // kLdBatch: the group's determinant product of event (t - t mod 8 + c)
    int bex = 0;

    // stream mode: this filter's event t is stream event e0 + t; one descriptor per stream
    // (events outside [0, S) are skipped: dropped loads, NONE type, dropped records)
    const int64_t e0 = STREAM ? (f % a.s_nchunks) * a.s_chunk + a.s_shift : 0;
    const uint32_t S = STREAM ? uint32_t(a.s_len) : 0u;
    const auto r_et = bytes_rsrc(a.etype, S), r_dt = bytes_rsrc(a.dt, S * 8u);
    const auto r_pay = bytes_rsrc(a.payload, S * 9u * uint32_t(sizeof(T)));
    // filter f is variant f / s_nchunks of its chunk (NV = 1) or carries variants 0 .. NV - 1:
    // with s_nvar > 1, variant q's trajectory records go to rows [q * s_vstride, q * s_vstride +
    // S) (s_vstride >= S + chunk, so a padded chunk's rows past S stay inside its own variant),
    // and only variant 0 writes the others
    const int var = STREAM ? int(f / a.s_nchunks) + vb : 0;
    const uint32_t trows = STREAM ? (a.s_nvar > 1 ? uint32_t(a.s_nvar) * uint32_t(a.s_vstride) : S) : 0u;
    const auto r_str = bytes_rsrc(a.traj, trows * uint32_t(M::NTRAJ * sizeof(T)));
    const auto r_scv = bytes_rsrc(a.cov, S * uint32_t(M::NBLK * sizeof(T)));
    const auto r_sld = bytes_rsrc(a.logdet, S * uint32_t(sizeof(T)));
    const auto r_sup = bytes_rsrc(a.updated, S);
    // Stream offsets are plain 32-bit products of ue = uint32(e): an event before the stream
    // start wraps far past every descriptor's length and one past its end lands beyond it, so
    // loads return 0 and stores drop without a select on the address (a select there was turned
    // into branches around the loads, whose joins drained the prefetch ring with vmcnt(0)).
    // Lanes without a record OR in bit 31 (kf_run_stream keeps (S + W) * rows * w < 2^31).
    const uint32_t m_tr = v_tr != kDropOffset ? 0u : kDropOffset;
    const uint32_t col_tr = v_tr != kDropOffset ? (uint32_t(var) * uint32_t(a.s_vstride) * M::NTRAJ + uint32_t(xi[0])) *
                                                      uint32_t(sizeof(T))
                                                : 0u;
    const uint32_t vstep_tr = uint32_t(a.s_vstride) * uint32_t(M::NTRAJ * sizeof(T));  // next variant's rows
    const uint32_t m_ld = c == 0 && var == 0 ? 0u : kDropOffset;  // variant 0's group only
    uint32_t col_cv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k)
        col_cv[k] = pr[k] >= 0 && var == 0 ? uint32_t(pr[k]) * uint32_t(sizeof(T)) : kDropOffset;
    auto load = [&](int t, ChainIn<T>& in) {
        if constexpr (STREAM) {
            const uint32_t ue = uint32_t(e0 + t);
            const int ty = int(__builtin_amdgcn_raw_buffer_load_b8(r_et, ue, 0, 0));
            in.type = ue < S ? ty : 255;
            in.dt = ldv(r_dt, ue * 8u, 0.0);
            in.va = ldv(r_pay, (ue * 9u + uint32_t(L.ia)) * uint32_t(sizeof(T)), T(0));
            in.vb = ldv(r_pay, (ue * 9u + uint32_t(L.ib)) * uint32_t(sizeof(T)), T(0));
        } else {
            in.type = int(ldb<uint8_t>(a.etype, t, uint32_t(a.B), uint32_t(f)));
            in.dt = ldb<double>(a.dt, t, rb8, off8);
            const auto rpay = span_rsrc(a.payload, int64_t(t) * 9, rb, 9);
            in.va = ldv(rpay, v_a, T(0));
            in.vb = ldv(rpay, v_b, T(0));
        }
    };
    auto step = [&](int t, const ChainIn<T>& in) {
        const bool applied = L.event(in.type, T(in.dt), in.va, in.vb, fg.on, gate, fg.thr, x, P, st);
        if constexpr (STREAM) {
            const uint32_t ue = uint32_t(e0 + t);
#pragma unroll
            for (int v = 0; v < NL; ++v)
                stv(r_str, (ue * uint32_t(M::NTRAJ * sizeof(T)) + col_tr + uint32_t(v) * vstep_tr) | m_tr, x[v][0]);
            // absent records: skipped by a wave-uniform branch (a store to a zero-length
            // descriptor is dropped, but it is still issued)
            if (a.cov) {
#pragma unroll
                for (int k = 0; k < 6; ++k)
                    stv(r_scv, (ue * uint32_t(M::NBLK * sizeof(T)) + col_cv[k]) | (col_cv[k] & kDropOffset), P[k]);
            }
            if (need_ld) {
                if constexpr (kLdBatch) {
                    T m;
                    int ex;
                    chain_det_mant(P, m, ex);
                    m = live ? m : T(1);
                    ex = live ? ex : 0;
                    group_prod(m, ex);
                    const int slot = t & (kGroup - 1);
                    if (c == slot) {
                        bm = m;
                        bex = ex;
                    }
                    if (slot == kGroup - 1 || t == a.T - 1) {  // wave-uniform: lane j logs event t - slot + j
                        int e;
                        const T ld = log_mant(frexp(bm, &e), bex + e);
                        const bool mine = c <= slot;
                        if (group_any(mine && !(ld == ld))) st = kNotSpd;
                        const uint32_t uj = uint32_t(e0 + t - slot + c);
                        stv(r_sld, (uj * uint32_t(sizeof(T))) | (mine && var == 0 ? 0u : kDropOffset), ld);
                    }
                } else {
                    const T ld = group_sum(live ? chain_log_det(P) : T(0));
                    st = (ld == ld) ? st : kNotSpd;
                    stv(r_sld, (ue * uint32_t(sizeof(T))) | m_ld, ld);
                }
            }
            if (a.updated) __builtin_amdgcn_raw_buffer_store_b8(applied ? uint8_t(1) : uint8_t(0), r_sup, ue | m_ld, 0, 0);
        } else {
            stv(span_rsrc(a.traj, int64_t(t) * M::NTRAJ, rb, M::NTRAJ), v_tr, x[0][0]);
            {
                const auto rc = span_rsrc(a.cov, int64_t(t) * M::NBLK, rb, M::NBLK);
#pragma unroll
                for (int k = 0; k < 6; ++k) stv(rc, vp[k], P[k]);
            }
            if (need_ld) {
                const T ld = group_sum(live ? chain_log_det(P) : T(0));
                st = (ld == ld) ? st : kNotSpd;
                stv(span_rsrc(a.logdet, t, rb, 1), v_ld, ld);
            }
            if (a.updated && c == 0) a.updated[int64_t(t) * a.B + f] = applied ? 1 : 0;
        }
    };

    constexpr int D = STREAM ? (NV > 1 ? kStreamVarDepth : kStreamDepth) : kChainDepth;
    const int T_ = a.T;
    ring_run<D, T>(T_, [&](int t, ChainIn<T>& in) { load(t < T_ ? t : T_ - 1, in); }, step);
    {
        const auto rx = span_rsrc(a.x, 0, rbank, M::N), rp = span_rsrc(a.P, 0, rbank, M::NBLK);
#pragma unroll
        for (int v = 0; v < NL; ++v)
#pragma unroll
            for (int k = 0; k < 3; ++k)
                stv(rx, vx[k] == kDropOffset ? kDropOffset : vx[k] + uint32_t(vb + v) * rb, x[v][k]);
        if (vb == 0) {
#pragma unroll
            for (int k = 0; k < 6; ++k) stv(rp, vp[k], P[k]);
        }
    }
    if (c == 0 && vb == 0) a.status[f] = st;
    if constexpr (NV == 4) {
        // the map pass's epilogue (kf_run_stream): this chunk's affine map per chain, x_end =
        // A x_start + b (fp64), A by differences of the variants (variant q + 1 started at the
        // guess + delta on component q), b = x_end(guess) - A guess; then the covariance seam:
        // this chunk's end covariance against the next chunk's start covariance, relative to
        // the end covariance's largest entry in the chain (one atomic per wave)
        constexpr int NCH = M::NP + M::NA;
        const int ns = pva ? 3 : 2;
        double crel = 0.0;
        // every variant's end state: with the split, variants 2, 3 come from the other group of
        // 16 (DPP row_ror:8 pairs lane l with l + 8 within the row), every lane exchanging
        double xe[4][3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
            for (int v = 0; v < NL; ++v) xe[v][k] = double(x[v][k]);
            if constexpr (NL < 4) {
#pragma unroll
                for (int v = 0; v < NL; ++v) xe[NL + v][k] = dpp_d<kDppRowRor8>(xe[v][k]);
            }
        }
        if (live && a.s_maps && vb == 0) {
            double A[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}, b[3] = {0, 0, 0};
            const double rdelta = 1.0 / a.s_delta;  // delta is a power of two: exact
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                if (k >= ns) continue;
                const double e0v = xe[0][k];
                double sacc = e0v;
#pragma unroll
                for (int qq = 0; qq < 3; ++qq) {
                    if (qq >= ns) continue;
                    A[k][qq] = (xe[qq + 1][k] - e0v) * rdelta;
                    sacc = __builtin_fma(-A[k][qq], double(xs0[qq]), sacc);
                }
                b[k] = sacc;
            }
            double* mo = a.s_maps + (f * NCH + c) * 12;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
#pragma unroll
                for (int qq = 0; qq < 3; ++qq) mo[k * 3 + qq] = A[k][qq];
                mo[9 + k] = b[k];
            }
            if (a.s_check && f + 1 < a.B) {
                double scale = 0.0, gap = 0.0;
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    if (pr[k] < 0) continue;
                    const double pe = double(P[k]);
                    scale = fmax(scale, fabs(pe));
                    gap = fmax(gap, fabs(pe - wnx[k]));
                }
                const double rel = gap / fmax(scale, 1e-300);
                crel = rel == rel ? rel : __builtin_inf();
            }
        }
        if (a.s_check) {
            // the wave's max over its chunks (DPP inside a group; lanes of finished groups hold
            // 0), one atomic per wave: every chunk's lanes finish together, and one atomic per
            // chunk on the same address queued up behind each other at the end of the pass
            crel = fmax(crel, dpp_d<kDppXor1>(crel));
            crel = fmax(crel, dpp_d<kDppXor2>(crel));
            crel = fmax(crel, dpp_d<kDppHalfMirror>(crel));
            // a wave whose chunks all exist has every lane here (a partial last wave lost its
            // dead groups at the top, so it keeps one atomic per chunk)
            const bool full = (g & ~int64_t(63)) / LPF + 64 / LPF <= a.B;  // wave-uniform
            if (full) {
#pragma unroll
                for (int sh = kGroup; sh < 64; sh <<= 1) crel = fmax(crel, __shfl_xor(crel, sh, 64));
                const bool lane0 = (threadIdx.x & 63) == 0;
                if (lane0 && crel != 0.0) atomic_max_pos(&a.s_check->cov_gap, crel);
                const bool any_bad = __builtin_amdgcn_ballot_w64(c == 0 && st != 0) != 0;
                if (lane0 && any_bad) atomicOr(&a.s_check->bad, kStreamBadFilter);
            } else {
                if (c == 0 && vb == 0 && crel != 0.0) atomic_max_pos(&a.s_check->cov_gap, crel);
                if (c == 0 && vb == 0 && st != 0) atomicOr(&a.s_check->bad, kStreamBadFilter);
            }
        }
    }
}

// ------------------------------------------------------------------------------------
// ONE gated filter (B = 1, the adaptive threshold, kf_workers.py:959-1058) whose gate blocks
// most updates, on one wave: lane c + 8 j is chain c (the chain kernel's lane layout) of event
// slot j.  Every event that applies an update runs as ChainLane::event, the same in every slot.
// After an event that did not, the wave looks ahead over the next 8 events at
// once: between two updates the filter only predicts, and with the model's additive F (F(a) F(b)
// = F(a + b)) and diagonal Q(dt) a run of predicts has a closed form,
//   P_m = F(tau_m) (P + S_m) F(tau_m)^T,  S_m = sum_{i <= m} F(-tau_i) Q(dt_i) F(-tau_i)^T,
// tau the time since the last event run (prefix sums over the slots), x_m = F(tau_m) x.  Slot j
// takes event t + j; the first slot whose event would open the gate (GateBand on its closed-form
// P_pred, a ballot over the slots) ends the run: the slots before it write their records at
// once and hand their state on, and that event runs next as a chain-kernel event.  The closed
// form rounds differently from one predict after another (records within 1.8e-12 relative of the
// chain kernel's over 70,000 events, every flag equal); a gate decision could only differ within
// that distance of the threshold (in f32 it does: f64 only).  KF_OPT_EVENTS_KERNEL = 4 runs it,
// and kf_run_events' gated one-filter route when the chunked run falls back after updating at
// most 1 event in 8 (launch_stream_choose).
// ------------------------------------------------------------------------------------
template <typename T, class M, bool CUSTOM>
__global__ __launch_bounds__(64) void ref_chain_gated_kernel(const RefArgs a) {
    if (a.skip && *a.skip) return;
    const int lane = int(threadIdx.x);
    const int slot = lane / kGroup;  // event slot of the look-ahead
    const ChainLane<T, M, CUSTOM> L(lane & (kGroup - 1), a.kc);
    const int c = L.c, ia = L.ia, ib = L.ib;
    const bool pva = L.pva, live = L.live;
    const auto& xi = L.xi;
    const auto& pr = L.pr;
    const auto& q = L.q;
    const T* hx = static_cast<const T*>(a.x);
    const T* hP = static_cast<const T*>(a.P);
    T x[1][3], P[6];
#pragma unroll
    for (int k = 0; k < 3; ++k) x[0][k] = xi[k] >= 0 ? hx[xi[k]] : T(0);
#pragma unroll
    for (int k = 0; k < 6; ++k) P[k] = pr[k] >= 0 ? hP[pr[k]] : L.unit(k);
    int32_t st = a.status[0];
    GateBand<T> gate;
    gate.init(a.threshold);
    const T thr = T(a.threshold);
    const T* pay = static_cast<const T*>(a.payload);
    const bool cov = a.cov != nullptr, ldo = a.logdet != nullptr;
    const int T_ = a.T;
    // an event step's records (t wave-uniform): slot 0's lanes write, through buffer stores whose
    // offsets drop the other slots' and the absent rows' stores (the chain kernel's form)
    constexpr uint32_t rb = uint32_t(sizeof(T));
    const uint32_t v_tr0 = slot == 0 && xi[0] >= 0 && xi[0] < M::NTRAJ ? uint32_t(xi[0]) * rb : kDropOffset;
    uint32_t vp0[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) vp0[k] = slot == 0 && pr[k] >= 0 ? uint32_t(pr[k]) * rb : kDropOffset;
    const uint32_t v_ld0 = slot == 0 && c == 0 ? 0u : kDropOffset;
    auto record_step = [&](int t, bool applied) {
        stv(span_rsrc(a.traj, int64_t(t) * M::NTRAJ, rb, M::NTRAJ), v_tr0, x[0][0]);
        if (cov) {
            const auto rc = span_rsrc(a.cov, int64_t(t) * M::NBLK, rb, M::NBLK);
#pragma unroll
            for (int k = 0; k < 6; ++k) stv(rc, vp0[k], P[k]);
        }
        if (ldo) {
            const T ld = group_sum(live ? chain_log_det(P) : T(0));
            st = (ld == ld) ? st : kNotSpd;
            stv(span_rsrc(a.logdet, t, rb, 1), v_ld0, ld);
        }
        if (slot == 0 && c == 0 && a.updated) a.updated[t] = applied ? 1 : 0;
    };
    // a look-ahead run's records (events t0 + slot for the slots < n; t0 wave-uniform): one
    // descriptor over the run's rows, each slot's lanes at their row, the other stores dropped
    const uint32_t v_trr = xi[0] >= 0 && xi[0] < M::NTRAJ ? uint32_t(slot * M::NTRAJ + xi[0]) * rb : kDropOffset;
    uint32_t vpr[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) vpr[k] = pr[k] >= 0 ? uint32_t(slot * M::NBLK + pr[k]) * rb : kDropOffset;
    const uint32_t v_ldr = c == 0 ? uint32_t(slot) * rb : kDropOffset;
    auto record_run = [&](int t0, int n, const T (&xr)[3], const T (&Pr)[6]) {
        const uint32_t wm = slot < n ? 0u : kDropOffset;
        const uint32_t rows = uint32_t(T_ - t0 < 8 ? T_ - t0 : 8);
        stv(span_rsrc(a.traj, int64_t(t0) * M::NTRAJ, rb, rows * M::NTRAJ), v_trr | wm, xr[0]);
        if (cov) {
            const auto rc = span_rsrc(a.cov, int64_t(t0) * M::NBLK, rb, rows * M::NBLK);
#pragma unroll
            for (int k = 0; k < 6; ++k) stv(rc, vpr[k] | wm, Pr[k]);
        }
        if (ldo) {
            const T ld = group_sum(live ? chain_log_det(Pr) : T(0));
            st = (ld == ld || slot >= n) ? st : kNotSpd;
            stv(span_rsrc(a.logdet, t0, rb, rows), v_ldr | wm, ld);
        }
        if (slot < n && c == 0 && a.updated) a.updated[t0 + slot] = 0;
    };
    int t = 0;
    // a look-ahead after an event that did not update, unless the last one found its run over at
    // once (then only after `cool` more such events: a regime of frequent updates stays on the
    // chain kernel's event step)
    int cool = 0, backoff = 0;
    // event t's inputs, loaded one event ahead (t + 1 while t runs; a look-ahead that moves t
    // reloads)
    int nt = 0;
    int ntype = T_ > 0 ? int(a.etype[0]) : 255;
    double ndt = T_ > 0 ? a.dt[0] : 0.0;
    T nva = T_ > 0 ? pay[ia] : T(0), nvb = T_ > 0 ? pay[ib] : T(0);
    while (t < T_) {  // wave-uniform
        // ---- event t, every slot the same arithmetic ----
        if (nt != t) {
            ntype = int(a.etype[t]);
            ndt = a.dt[t];
            nva = pay[int64_t(t) * 9 + ia];
            nvb = pay[int64_t(t) * 9 + ib];
        }
        const int type = ntype;
        const T dt = T(ndt);
        const T va = nva, vb = nvb;
        nt = t + 1;
        if (nt < T_) {
            ntype = int(a.etype[nt]);
            ndt = a.dt[nt];
            nva = pay[int64_t(nt) * 9 + ia];
            nvb = pay[int64_t(nt) * 9 + ib];
        }
        const bool applied = L.event(type, dt, va, vb, true, gate, thr, x, P, st);
        record_step(t, applied);
        ++t;
        // every lane holds the same decision (the gate's group ops, every slot the same event), but
        // the compiler cannot know it: taken from lane 0, so that t and the loop stay scalar (a
        // per-lane `continue` made t divergent, and with it every event's type branches)
        if (__builtin_amdgcn_readfirstlane(int(applied)) || t >= T_) continue;
        if (cool > 0) {
            --cool;
            continue;
        }
        for (;;) {  // look-aheads until a run ends (or the stream does)
        // ---- look-ahead: slot j predicts to event t + j in closed form ----
        const int e = t + slot;
        const bool valid = e < T_;
        const int ty = valid ? int(a.etype[e]) : 255;
        const bool pred = valid && ty != 255;
        const T dte = pred ? T(a.dt[e]) : T(0);
        // tau: time since event t - 1 up to and including slot j's event (prefix over slots)
        T tau = dte;
#pragma unroll
        for (int o = 1; o < 8; o *= 2) {
            const T u = __shfl_up(tau, o * kGroup, 64);
            tau += slot >= o ? u : T(0);
        }
        // this slot's term F(-tau) Q(dt) F(-tau)^T (G = F(-tau): rows (1, -tau, h'), (0, 1, g'), (0, 0, 1))
        const T hm = pva ? T(0.5) * tau * tau : T(0), gm = pva ? -tau : T(0);
        const T d0 = q[0] * dte, d1 = q[1] * dte, d2 = q[2] * dte;
        T Sx[6];
        Sx[0] = fmaT(hm * hm, d2, fmaT(tau * tau, d1, d0));
        Sx[1] = fmaT(hm * gm, d2, -tau * d1);
        Sx[2] = hm * d2;
        Sx[3] = fmaT(gm * gm, d2, d1);
        Sx[4] = gm * d2;
        Sx[5] = d2;
#pragma unroll
        for (int o = 1; o < 8; o *= 2)
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const T u = __shfl_up(Sx[k], o * kGroup, 64);
                Sx[k] += slot >= o ? u : T(0);
            }
        // P_pred = F(tau) (P + S) F(tau)^T, F = [[1, tau, h], [0, 1, g], [0, 0, 1]]
        const T h = pva ? T(0.5) * tau * tau : T(0), g = pva ? tau : T(0);
        T A[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) A[k] = P[k] + Sx[k];
        T B[3][3];  // F A
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            B[0][j] = fmaT(h, A[tri<3>(2, j)], fmaT(tau, A[tri<3>(1, j)], A[tri<3>(0, j)]));
            B[1][j] = fmaT(g, A[tri<3>(2, j)], A[tri<3>(1, j)]);
            B[2][j] = A[tri<3>(2, j)];
        }
        T Pp[6];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) {
                T s = B[i][j];
                if (j == 0) s = fmaT(B[i][2], h, fmaT(B[i][1], tau, s));
                if (j == 1) s = fmaT(B[i][2], g, s);
                Pp[tri<3>(i, j)] = s;
            }
        if (!pva) Pp[5] = P[5];  // the inert state of an aw lane
        T xp[3] = {fmaT(h, x[0][2], fmaT(tau, x[0][1], x[0][0])), fmaT(g, x[0][2], x[0][1]), x[0][2]};
        const bool opens = valid && (ty == kGps || ty == kImu) && gate.open(Pp, live, thr);
        const uint64_t om = __builtin_amdgcn_ballot_w64(opens && c == 0);
        const int nvalid = T_ - t < 8 ? T_ - t : 8;
        const int n = om ? int(__builtin_ctzll(om)) / kGroup : nvalid;  // events of the predict run
        record_run(t, n, xp, Pp);
        st = __builtin_amdgcn_ballot_w64(st == kNotSpd) ? kNotSpd : st;  // a failed record in any slot
        if (n > 0) {
            const int src = (n - 1) * kGroup + c;
#pragma unroll
            for (int k = 0; k < 3; ++k) x[0][k] = __shfl(xp[k], src, 64);
#pragma unroll
            for (int k = 0; k < 6; ++k) P[k] = __shfl(Pp[k], src, 64);
            t += n;
        }
        if (n < 4 && om) {  // a short run: look-aheads do not pay here, back off
            backoff = backoff ? (backoff < 32 ? 2 * backoff : 32) : 1;
            cool = backoff;
        } else if (n >= 4) {
            backoff = 0;
        }
        if (om || n < 8 || t >= T_) break;  // the run ended (its opening event runs next) or the stream did
        }
    }
    if (slot == 0) {
        T* ox = static_cast<T*>(a.x);
        T* oP = static_cast<T*>(a.P);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (xi[k] >= 0) ox[xi[k]] = x[0][k];
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (pr[k] >= 0) oP[pr[k]] = P[k];
        if (c == 0) a.status[0] = st;
    }
}

template <typename T, class M, bool CUSTOM>
void ref_events_chain_t(const RefArgs& a, hipStream_t stream, int variant) {
    if (variant == kEventsGated) {  // no per-filter gates: launch_ref_events refuses a.thresholds here
        ref_chain_gated_kernel<T, M, CUSTOM><<<1, 64, 0, stream>>>(a);
        return;
    }
    const dim3 cgrid(static_cast<unsigned>((a.B * kGroup + kBlock - 1) / kBlock));
    KF_BOOL_DISPATCH(a.thresholds, GATES, ref_chain_kernel<T, M, false, CUSTOM, 1, GATES><<<cgrid, kBlock, 0, stream>>>(a));
}
template <typename T, class M, bool CUSTOM>
void ref_stream_t(const RefArgs& a, hipStream_t stream, int nv) {
    if (nv == 4) {
        const dim3 vgrid(static_cast<unsigned>((a.B * chain_lanes<4>() + kBlock - 1) / kBlock));
        ref_chain_kernel<T, M, true, CUSTOM, 4><<<vgrid, kBlock, 0, stream>>>(a);
    } else {
        const dim3 cgrid(static_cast<unsigned>((a.B * kGroup + kBlock - 1) / kBlock));
        ref_chain_kernel<T, M, true, CUSTOM><<<cgrid, kBlock, 0, stream>>>(a);
    }
}
}  // namespace

hipError_t launch_ref_events_chain(int model, bool f64, const RefArgs& a, hipStream_t stream, int variant) {
    KF_REF_DISPATCH(model, f64, a.kc, ref_events_chain_t<T, M, CUSTOM>(a, stream, variant));
    return hipGetLastError();
}

hipError_t launch_ref_stream(int model, bool f64, const RefArgs& a, hipStream_t stream, int nv) {
    if (a.s_len <= 0 || a.s_nchunks <= 0 || (nv != 1 && nv != 4)) return hipErrorInvalidValue;
    if (model != 15 && model != 8) return hipErrorInvalidValue;
    KF_REF_DISPATCH(model, f64, a.kc, ref_stream_t<T, M, CUSTOM>(a, stream, nv));
    return hipGetLastError();
}

}  // namespace kfmi

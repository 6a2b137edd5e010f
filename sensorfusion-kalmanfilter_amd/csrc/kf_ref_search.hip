// The brute-force search over event subsets of the 15-state model (kf_ref_model.h): one filter
// per subset (kf_eval_combos: launch_ref15_combos) and the shared-prefix search by levels
// (kf_search_combos, kf_search_windows: the launch_ref15_search* launchers, set_search_band,
// launch_search_finish, launch_search_windows_finish).
#include "kf_ref_model.h"

namespace kfmi {
namespace {

// ------------------------------------------------------------------------------------
// Brute-force combination search (kf_eval_combos).  The n candidate events and the binomial
// table sit in LDS; lane f unranks combination combo_offset + f (lexicographic =
// itertools.combinations order) one index at a time while it runs the filter, so no per-lane
// index list is stored.
// ------------------------------------------------------------------------------------
#ifndef KF_COMBO_WAVES
#define KF_COMBO_WAVES 3  // waves per SIMD the one-filter-per-subset kernel is compiled for
#endif
template <typename T, bool CUSTOM>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(KF_COMBO_WAVES))) void ref15_combo_kernel(
    const Ref15ComboArgs a) {
    __shared__ double s_ev[kMaxEvents * 11];
    __shared__ uint64_t s_binom[(kMaxEvents + 1) * (kMaxEvents + 1)];
    const int n = a.n_events;
    for (int i = threadIdx.x; i < n * 11; i += kBlock) s_ev[i] = a.ev[i];
    for (int i = threadIdx.x; i < (n + 1) * (kMaxEvents + 1); i += kBlock) s_binom[i] = a.binom[i];
    __syncthreads();

    const int64_t f = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (f >= a.B) return;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(a.B) * uint32_t(sizeof(T));
    const uint64_t rank0 = a.combo_offset + uint64_t(f);
    const bool live = rank0 < a.n_combos;
    // records land at a per-lane row (a skipped event shifts them): one span over the k+2 rows
    const auto r_ld = span_rsrc(a.logdets, 0, rb, uint32_t(a.k + 2));

    Ref15<T, CUSTOM> s;
    s.kc = a.kc;
#pragma unroll
    for (int i = 0; i < 15; ++i) s.x[i] = T(a.init[i]);
#pragma unroll
    for (int r = 0; r < 27; ++r) s.blk(r) = T(a.init[15 + r]);

    // record 0: logdet of the initial covariance (kf_workers.py:32)
    T ld = s.logdet();
    T ld_max = ld;
    int rec = 0;
    stv(r_ld, uint32_t(rec) * rb + off, ld);
    ++rec;
    bool ok = true;
    double cur = a.prev_time;
    uint64_t r = live ? rank0 : 0;
    int cand = 0;
    const T no_gate = T(0);
    for (int j = 0; j < a.k; ++j) {
        // unrank the j-th element: skip candidates whose sub-tree is entirely below r
        const int left = a.k - j - 1;
        while (cand < n) {
            const uint64_t cnt = s_binom[(n - cand - 1) * (kMaxEvents + 1) + left];
            if (r < cnt) break;
            r -= cnt;
            ++cand;
        }
        const int e = cand < n ? cand : n - 1;
        ++cand;
        const double te = s_ev[e * 11];
        const double dtd = te - cur;
        if (dtd < 0.0) continue;  // kf_workers.py:38-40: skip, prev time unchanged
        T pay[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) pay[i] = T(s_ev[e * 11 + 2 + i]);
        s.event(int(s_ev[e * 11 + 1]), T(dtd), pay, false, no_gate, ok);
        cur = te;
        ld = s.logdet();
        ld_max = ld > ld_max ? ld : ld_max;
        stv(r_ld, uint32_t(rec) * rb + off, ld);
        ++rec;
    }
    // always propagate to the common end time (kf_workers.py:74-82)
    if (cur < a.target_end - 1e-8) {
        s.predict(T(a.target_end - cur));
        ld = s.logdet();
        ld_max = ld > ld_max ? ld : ld_max;
        stv(r_ld, uint32_t(rec) * rb + off, ld);
        ++rec;
    }
    for (int q = rec; q < a.k + 2; ++q) stv(r_ld, uint32_t(q) * rb + off, quiet_nan<T>());
    int32_t st = ok ? 0 : kNotSpd;
    if (!live) {
        st = 1;
        ld_max = quiet_nan<T>();
    } else if (!ok || !(ld_max == ld_max)) {
        st = kNotSpd;
        s.fill_nan();
        ld_max = quiet_nan<T>();
    }
    if (a.max_logdet) stb(a.max_logdet, 0, rb, off, ld_max);
    if (a.n_records) a.n_records[f] = rec;
    s.store(a.x, a.P, rb, off);
    a.status[f] = st;
}

// ------------------------------------------------------------------------------------
// Brute-force search with shared prefixes (kf_search_combos).  The worker runs every subset's
// filter from the common start (kf_workers.py:29-71), so a k-subset repeats all of the work of
// its (k-1)-prefix: over all subsets of n events that is ~n/2 + 1 event steps per subset.  Here
// the filter of subset S = P + {j} (j > max P) is P's stored filter advanced by event j — the
// same operations in the same order as the per-combination kernel, so the same numbers — and
// each subset costs one event step plus the worker's final predict (:74-82).
//
// One lane per parent P (level k - 1, colex order).  Its children j = max P + 1 .. n - 1 are
// visited in a wave-uniform loop: parents of a wave share max P except at run boundaries, so
// event j is the same for every active lane (scalar loads, uniform GPS/IMU branch), and for a
// fixed j the children of consecutive parents are consecutive ranks (coalesced stores).
// ------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint64_t o = __shfl_xor(v, s, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

// Level buffers in node blocks of 64 (kf_internal.h): a wave's parents are one contiguous block.
template <typename T, bool SYM = false>
__device__ __forceinline__ char* level_block(const void* base, uint64_t c) {
    return static_cast<char*>(const_cast<void*>(base)) + (c >> 6) * search_block_bytes(sizeof(T), SYM);
}
template <typename T>
__device__ __forceinline__ T* level_row(char* blk, uint32_t lane, int r) {
    return reinterpret_cast<T*>(blk + r * 64 * int(sizeof(T))) + lane;
}
// the running max's binary exponent (int32 per node, after the T rows)
template <typename T, bool SYM = false>
__device__ __forceinline__ int32_t* level_exp(char* blk, uint32_t lane) {
    return reinterpret_cast<int32_t*>(blk + search_rows(SYM) * 64 * int(sizeof(T))) + lane;
}
template <typename T, bool SYM = false>
__device__ __forceinline__ double* level_tail(char* blk, uint32_t lane, int q) {
    return reinterpret_cast<double*>(blk + search_rows(SYM) * 64 * int(sizeof(T)) + 256 + q * 512) + lane;
}

// A positive determinant as (mantissa in [0.5, 1), binary exponent); a failed filter's has a NaN
// mantissa.  The search carries each subset's running max this way and compares determinants,
// not their logs (log is monotone): one log per scored subset where its max log-det is an
// output (subset_max), none where only the acceptance test reads it (DetBand), instead of a log
// per record and per final predict.
// A NaN determinant carries the exponent that makes the comparisons below treat it as the log
// domain's `ld > run ? ld : run` treats a NaN: kNanLoses on a failed record or final predict
// (it never wins a max), kNanWins on a failed running max (nothing beats it: it stays NaN).
constexpr int kNanLoses = -2147483647 - 1, kNanWins = 2147483647;
template <typename T>
struct DetV {
    T m;
    int e;
    __device__ __forceinline__ bool valid() const { return m == m; }
    // this > o (by exponent, then mantissa: both normalised)
    __device__ __forceinline__ bool gt(const DetV& o) const { return e > o.e || (e == o.e && m > o.m); }
    __device__ __forceinline__ T log() const { return valid() ? log_mant(m, e) : quiet_nan<T>(); }
    __device__ __forceinline__ void fail() {
        m = quiet_nan<T>();
        e = kNanWins;
    }
};

// `d.gt(r) ? d : r`, the exponent blended with a mask (a select of two loaded members is folded
// into a load from a select of their addresses, which keeps the search node in scratch memory)
template <typename T>
__device__ __forceinline__ DetV<T> dmax(const DetV<T>& d, const DetV<T>& r) {
    const bool g = d.gt(r);
    const int mk = -int(g);
    return DetV<T>{g ? d.m : r.m, (d.e & mk) | (r.e & ~mk)};
}

// The acceptance test max(log_det) < R_threshold (kf_workers.py:1353) on a determinant: below
// lo it holds and above hi it fails for any log the kernels could compute (lo, hi = exp(thr) (1
// -+ eps), eps far above log_mant's and exp's rounding near thr; set_search_band computes them
// on the host); in between the log decides, as `log < T(thr)` exactly.
template <typename T>
struct DetBand {
    DetV<T> lo, hi;
    // 0: the band; 1: accept every valid determinant; 2: accept only a valid determinant that
    // underflowed to 0 (log -inf, below any finite threshold); 3: accept none (-inf or NaN)
    int mode;
    T thr;
    __device__ __forceinline__ explicit DetBand(const Ref15SearchArgs& a)
        : lo{T(a.band_lo_m), a.band_lo_e}, hi{T(a.band_hi_m), a.band_hi_e}, mode(a.band_mode), thr(T(a.threshold)) {}
    // d: a subset's max (valid, or NaN with kNanWins, which lies above hi)
    __device__ __forceinline__ bool accept(const DetV<T>& d) const {
        if (mode != 0) return d.valid() && (mode == 1 || (mode == 2 && d.m == T(0)));
        if (lo.gt(d)) return true;
        if (d.gt(hi)) return false;
        return log_mant(d.m, d.e) < thr;
    }
};

// Chains<T, M15>::logdet() accumulated one block at a time, in its order (pva chains, then aw
// chains) with its renormalisations, so the value is the same.
template <typename T>
struct LogdetAcc {
    T num = T(1), den = T(1);
    int ex = 0;
    bool ok = true;
    __device__ __forceinline__ void add_pva(const T (&P)[6], int c) {
        det3_scaled<T>(P, num, den, ok);
        if (sizeof(T) == 4 || c == M15::NP - 1) renorm(num, ex);
    }
    __device__ __forceinline__ void add_aw(const T (&P)[3]) {
        det2<T>(P, num, ok);
        if (sizeof(T) == 4) renorm(num, ex);
    }
    __device__ __forceinline__ T finish() {
        T prod = num * rcp_nr<kRefNewton>(den);
        renorm(prod, ex);
        const T ld = log_mant(prod, ex);
        return ok ? ld : quiet_nan<T>();
    }
    // the determinant itself (Chains::det_mant's value): no log.  A product that underflowed to 0
    // (log -inf) takes the lowest exponent, so it orders below every positive determinant.
    __device__ __forceinline__ DetV<T> det() {
        T prod = num * rcp_nr<kRefNewton>(den);
        renorm(prod, ex);
        return DetV<T>{ok ? prod : quiet_nan<T>(), ok && prod != T(0) ? ex : kNanLoses};
    }
};

// A stored node of the search: the covariance after a subset's events, its running max
// determinant (DetV: the max log-det before its log), the time of its last applied event and its
// subset mask.  The search scores a subset
// by its max log-det alone, which depends on the covariance alone, and the covariance does not
// depend on the measurements (nor, so, on the state): the state is not carried (kf_eval_combos
// carries it for the per-combination API).  The updates see a constant zero state (search_pva,
// search_aw), so their state half is dead code the compiler removes.
// SYM (Ref15SearchArgs::sym): the three pva chains, and the three aw chains, have the same
// constants and the same start, so in exact arithmetic the same covariance; the node holds one of
// each (rows 0..5 pva, 6..8 aw) and the search computes one of each, entering it into the
// log-dets once per chain it stands for.  (The every-chain kernels' separately compiled copies
// of a chain round alike in most subsets and one ulp apart in some.)
template <typename T, bool CUSTOM, bool SYM = false>
struct SearchNode {
    static constexpr int NP = SYM ? 1 : M15::NP, NA = SYM ? 1 : M15::NA;
    static constexpr int NR = 6 * NP + 3 * NA;  // covariance rows held (27, or 9)
    T P[NR];
    DetV<T> run;
    double prev;
    uint64_t mask;

    // The root (defined after search_child_to, whose operations it applies to the fixed events)
    __device__ __forceinline__ DetV<T> root(const Ref15SearchArgs& a, bool eval);
    __device__ __forceinline__ void load(const void* level, uint64_t p) {
        char* blk = level_block<T, SYM>(level, p);
        const uint32_t lane = uint32_t(p) & 63u;
#pragma unroll
        for (int i = 0; i < NR; ++i) P[i] = *level_row<T>(blk, lane, i);
        run.m = *level_row<T>(blk, lane, NR);
        run.e = *level_exp<T, SYM>(blk, lane);
        prev = *level_tail<T, SYM>(blk, lane, 0);
        mask = __builtin_bit_cast(uint64_t, *level_tail<T, SYM>(blk, lane, 1));
    }
    // the node as level K + 1's parent at colex rank r (the head kernel)
    __device__ __forceinline__ void store(void* level, uint64_t r) const {
        char* cb = level_block<T, SYM>(level, r);
        const uint32_t cl = uint32_t(r) & 63u;
#pragma unroll
        for (int i = 0; i < NR; ++i) *level_row<T>(cb, cl, i) = P[i];
        *level_row<T>(cb, cl, NR) = run.m;
        *level_exp<T, SYM>(cb, cl) = run.e;
        *level_tail<T, SYM>(cb, cl, 0) = prev;
        *level_tail<T, SYM>(cb, cl, 1) = __builtin_bit_cast(double, mask);
    }
    // largest free candidate in the subset (local index), -1 for the root
    __device__ __forceinline__ int max_event(int shift) const {
        const uint64_t loc = mask >> shift;
        return loc ? 63 - __builtin_clzll(loc) : -1;
    }
};

// a scored subset: every max log-det to subset_max (its one log), the acceptance test into
// (best, cnt) — on the determinant (DetBand) when no log was taken
template <typename T>
__device__ __forceinline__ void search_score(const Ref15SearchArgs& a, const DetBand<T>& band, uint64_t mask,
                                             const DetV<T>& fmax, uint64_t& best, uint64_t& cnt) {
    bool acc;
    if (a.subset_max) {
        const T ld = fmax.log();
        static_cast<T*>(a.subset_max)[mask] = ld;
        acc = ld < band.thr;
    } else {
        acc = band.accept(fmax);
    }
    if (acc) {  // max(log_det) < R_threshold (kf_workers.py:1353); NaN never passes
        const uint64_t key = __builtin_bitreverse64(mask);  // larger key = earlier in itertools order
        best = key > best ? key : best;
        ++cnt;
    }
}

// Event j applied to a node whose last applied event is at prev_in (kf_workers.py:36-82): a
// negative dt skips the event and keeps the time; the worker's final predict to target_end runs
// when the new time is before it.
// the search's events are read through ro() (the table above `ro`): scalar loads in the child loops
struct SearchEvent {
    ro_double* e;
    int type;
    bool step, final_predict;
    double dt, dte, prev;  // prev: the time after the event
};

__device__ __forceinline__ SearchEvent search_event(const Ref15SearchArgs& a, int j, double prev_in) {
    SearchEvent v;
    v.e = ro(a.ev) + j * 11;
    v.type = int(v.e[1]);
    v.dt = v.e[0] - prev_in;
    v.step = v.dt >= 0.0;  // kf_workers.py:38-40
    v.prev = v.step ? v.e[0] : prev_in;
    v.final_predict = v.prev < a.target_end - 1e-8;  // kf_workers.py:74-82
    v.dte = a.target_end - v.prev;
    return v;
}

// One chain of the 15-state filter through one event, Chains::event's operations for that
// chain (each chain's predict and update touch only that chain); the state is not carried
// (SearchNode), so xb is constant zeros and the state half is dead code after inlining.
template <typename T, bool CUSTOM>
__device__ __forceinline__ void search_pva(const SearchEvent& v, int ch, T (&Pb)[6], bool& ok, const RefConsts* kc) {
    using C15 = Chains<T, M15>;
    T qpva[3], Rp[6], rg;
    pva_noise<CUSTOM, M15>(kc, ch, qpva, Rp, rg);
    const T Rg[1] = {rg};
    if (!v.step) return;
    const T dt = T(v.dt);
    T xb[3] = {T(0), T(0), T(0)};
    C15::template chain_predict<3>(xb, Pb, dt, qpva);
    if (v.type == kGps) {
        const T zb[1] = {T(v.e[2 + ch])};
        ok = sel_update<3, 1, true, T, kRefNewton, true, kRefJoseph<T>, kRefGainR>(xb, Pb, zb, Rg) && ok;
    } else {
        const T acc = T(v.e[2 + M15::imu_acc(ch)]);
        const T V = fmaT(acc, dt, xb[1]);
        const T X = fmaT(V, dt, xb[0]);
        const T zb[3] = {X, V, acc};
        ok = sel_update<3, 3, true, T, kRefNewton, true, kRefJoseph<T>, kRefGainR>(xb, Pb, zb, Rp) && ok;
    }
}

template <typename T, bool CUSTOM>
__device__ __forceinline__ void search_aw(const SearchEvent& v, int ch, T (&Pa)[3], bool& ok, const RefConsts* kc) {
    using C15 = Chains<T, M15>;
    T qaw[2], Ra[3];
    aw_noise<CUSTOM, M15>(kc, ch, qaw, Ra);
    if (!v.step) return;
    T xa[2] = {T(0), T(0)};
    C15::template chain_predict<2>(xa, Pa, T(v.dt), qaw);
    if (v.type != kGps) {  // a GPS fix updates the pva chains only
        const T za[2] = {T(v.e[2 + M15::imu_att(ch)]), T(v.e[2 + M15::imu_rate(ch)])};
        ok = sel_update<2, 2, true, T, kRefNewton, true, kRefJoseph<T>, kRefGainR>(xa, Pa, za, Ra) && ok;
    }
}

// The log-dets of one subset: its record after the event (rec) and after the worker's final
// predict (fin), accumulated chain by chain in Chains::logdet's block order, so the numbers are
// kf_eval_combos's.
template <typename T, bool CUSTOM>
struct SearchScore {
    LogdetAcc<T> rec, fin;
    bool ok = true;
    const RefConsts* kc = nullptr;
    // chains ch .. ch + reps - 1 all holding Pb (reps = 3: the axis-symmetric search's one pva
    // chain standing for the three; their blocks enter the log-dets in the same order)
    __device__ __forceinline__ void add_pva(const SearchEvent& v, const T (&Pb)[6], int ch, int reps = 1) {
        using C15 = Chains<T, M15>;
        T qpva[3], Rp[6], rg;
        pva_noise<CUSTOM, M15>(kc, ch, qpva, Rp, rg);
#pragma unroll
        for (int r = 0; r < reps; ++r) rec.add_pva(Pb, ch + r);
        T Pf[6], xf[3] = {T(0), T(0), T(0)};
#pragma unroll
        for (int i = 0; i < 6; ++i) Pf[i] = Pb[i];
        C15::template chain_predict<3>(xf, Pf, T(v.dte), qpva);  // read by finish() only with v.final_predict
#pragma unroll
        for (int r = 0; r < reps; ++r) fin.add_pva(Pf, ch + r);
    }
    __device__ __forceinline__ void add_aw(const SearchEvent& v, const T (&Pa)[3], int ch, int reps = 1) {
        using C15 = Chains<T, M15>;
        T qaw[2], Ra[3];
        aw_noise<CUSTOM, M15>(kc, ch, qaw, Ra);
#pragma unroll
        for (int r = 0; r < reps; ++r) rec.add_aw(Pa);
        T Pf[3], xf[2] = {T(0), T(0)};
#pragma unroll
        for (int i = 0; i < 3; ++i) Pf[i] = Pa[i];
        C15::template chain_predict<2>(xf, Pf, T(v.dte), qaw);  // read by finish() only with v.final_predict
#pragma unroll
        for (int r = 0; r < reps; ++r) fin.add_aw(Pf);
    }
    // the running max determinant after the event (NaN for a failed filter, kf_eval_combos:
    // KF_ENOTSPD), and into fmax the subset's max with the final predict — the max log-dets'
    // determinants, no log taken
    __device__ __forceinline__ DetV<T> finish(const SearchEvent& v, const DetV<T>& run_in, DetV<T>& fmax) {
        DetV<T> run = run_in;
        if (v.step) {
            const DetV<T> d = rec.det();
            run = dmax(d, run_in);
            if (!ok) run.fail();
        }
        fmax = run;
        if (v.final_predict) {
            const DetV<T> d = fin.det();
            fmax = dmax(d, run);
        }
        return run;
    }
};

// Child j (> the parent's largest event) of node `par`, colex rank c at level a.k: scored into
// (best, cnt), and stored when a.child is set and the child has stored children (largest event
// <= n - 3).  With a.tail, the child holding event n - 2 is not stored: its only child (it plus
// event n - 1, level k + 1) is evaluated from the registers and scored into (best1, cnt1).
// Chain by chain: a chain's child covariance is stored (or carried through event n - 1) as soon
// as it is computed, so only one chain of the child and grandchild is live at a time.
// The parent's covariance as search_child reads it: from registers, or from a lane's LDS column
// (the parent-major kernel's LDS variant, which frees the registers that hold it across the
// loop over children).
// kChainFence: a scheduling barrier after each chain, so the compiler does not hoist the next
// chains' LDS reads over this one's arithmetic (which spilled the 3-wave LDS variant)
template <typename T>
struct ParRegs {
    static constexpr bool kChainFence = false;
    const T* P;
    __device__ __forceinline__ T operator()(int i) const { return P[i]; }
};
template <typename T>
struct ParLds {
    static constexpr bool kChainFence = true;
    const T* col;  // row i at col[i * 64]
    __device__ __forceinline__ T operator()(int i) const { return col[i * 64]; }
};

// Where search_child_to puts the child it computed: a level buffer's node (LevelSink: level k,
// stored for the next launch), or a lane's LDS column and registers (LdsSink: the pair kernel's
// level k, read back at once as the parent of level k + 1).  Either way the bits are the same.
template <typename T, bool SYM>
struct LevelSink {
    char* cb;
    uint32_t cl;
    bool on;
    __device__ __forceinline__ void row(int i, T v) const { *level_row<T>(cb, cl, i) = v; }
    __device__ __forceinline__ void node(int nr, const DetV<T>& run, double prev, uint64_t mask) const {
        *level_row<T>(cb, cl, nr) = run.m;
        *level_exp<T, SYM>(cb, cl) = run.e;
        *level_tail<T, SYM>(cb, cl, 0) = prev;
        *level_tail<T, SYM>(cb, cl, 1) = __builtin_bit_cast(double, mask);
    }
};
template <typename T>
struct LdsSink {
    T* col;  // row i at col[i * 64]
    bool on;
    DetV<T> run;
    double prev;
    uint64_t mask;
    __device__ __forceinline__ void row(int i, T v) const { col[i * 64] = v; }
    __device__ __forceinline__ void node(int, const DetV<T>& r, double p, uint64_t m) {
        run = r;
        prev = p;
        mask = m;
    }
};

// A class root's prefix nodes (SearchNode::root): the child's rows and scalars in registers,
// with its score's determinant (fmax) instead of a scoring
template <typename T, int NR>
struct RegSink {
    T P[NR];
    bool on;
    DetV<T> run, fmax;
    double prev;
    uint64_t mask;
    __device__ __forceinline__ void row(int i, T v) { P[i] = v; }
    __device__ __forceinline__ void node(int, const DetV<T>& r, double p, uint64_t m) {
        run = r;
        prev = p;
        mask = m;
    }
};

// SCORE = false: the child is not scored (nor is a tail computed); its max with the final predict
// goes to sk.fmax (RegSink)
template <typename T, bool CUSTOM, bool SYM, class PS, class SK, bool SCORE = true>
__device__ __forceinline__ void search_child_to(const Ref15SearchArgs& a, const DetBand<T>& band,
                                                const SearchNode<T, CUSTOM, SYM>& par, const PS& pp, int j, SK& sk,
                                                bool tail, uint64_t& best, uint64_t& cnt, uint64_t& best1,
                                                uint64_t& cnt1) {
    using Node = SearchNode<T, CUSTOM, SYM>;
    constexpr int RP = SYM ? M15::NP : 1, RA = SYM ? M15::NA : 1;  // chains each computed one stands for
    const SearchEvent vs = search_event(a, j, par.prev);
    const bool store = sk.on;
    SearchEvent vg;
    if (tail) vg = search_event(a, j + 1, vs.prev);
    SearchScore<T, CUSTOM> ss, sg;
    ss.kc = sg.kc = a.kc;
#pragma unroll
    for (int ch = 0; ch < Node::NP; ++ch) {
        T Pb[6];
#pragma unroll
        for (int i = 0; i < 6; ++i) Pb[i] = pp(6 * ch + i);
        search_pva<T, CUSTOM>(vs, ch, Pb, ss.ok, a.kc);
        if (store) {
#pragma unroll
            for (int i = 0; i < 6; ++i) sk.row(6 * ch + i, Pb[i]);
        }
        ss.add_pva(vs, Pb, ch, RP);
        if (tail) {
            search_pva<T, CUSTOM>(vg, ch, Pb, sg.ok, a.kc);
            sg.add_pva(vg, Pb, ch, RP);
        }
        if constexpr (PS::kChainFence) __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int ch = 0; ch < Node::NA; ++ch) {
        T Pa[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) Pa[i] = pp(6 * Node::NP + 3 * ch + i);
        search_aw<T, CUSTOM>(vs, ch, Pa, ss.ok, a.kc);
        if (store) {
#pragma unroll
            for (int i = 0; i < 3; ++i) sk.row(6 * Node::NP + 3 * ch + i, Pa[i]);
        }
        ss.add_aw(vs, Pa, ch, RA);
        if (tail) {
            search_aw<T, CUSTOM>(vg, ch, Pa, sg.ok, a.kc);
            sg.add_aw(vg, Pa, ch, RA);
        }
        if constexpr (PS::kChainFence) __builtin_amdgcn_sched_barrier(0);
    }
    DetV<T> fmax;
    const DetV<T> run = ss.finish(vs, par.run, fmax);
    const uint64_t cmask = par.mask | (uint64_t(1) << (j + a.shift));
    if (store) sk.node(Node::NR, run, vs.prev, cmask);
    if constexpr (SCORE) {
        search_score(a, band, cmask, fmax, best, cnt);
        if (tail) {
            DetV<T> gmax;
            (void)sg.finish(vg, run, gmax);
            search_score(a, band, cmask | (uint64_t(1) << (j + 1 + a.shift)), gmax, best1, cnt1);
        }
    } else {
        sk.fmax = fmax;
    }
}

// The root: the search's fixed events (a.root_mask, none for a whole search) applied to the
// initial filter in index order as the worker applies a combination's events
// (kf_workers.py:36-71); record 0 is the logdet of the initial covariance (:32).  Each fixed
// event is applied with search_child_to's operations, from the node its predecessors made, so a
// class root is bit for bit the node the whole search computes for that subset (its prefixes are
// not scored: they belong to other classes).  With `eval`, returns the root subset's max log-det
// with the final predict (as a determinant) for the caller to score.
template <typename T, bool CUSTOM, bool SYM>
__device__ __forceinline__ DetV<T> SearchNode<T, CUSTOM, SYM>::root(const Ref15SearchArgs& a, bool eval) {
    Ref15<T, CUSTOM> r;
    r.kc = a.kc;
#pragma unroll
    for (int i = 0; i < 15; ++i) r.x[i] = T(a.init[i]);
#pragma unroll
    for (int i = 0; i < 27; ++i) r.blk(i) = T(a.init[15 + i]);
    run.m = r.det_mant(run.e);
    if (!run.valid()) run.fail();
    if (run.m == T(0)) run.e = kNanLoses;
    prev = a.prev_time;
    mask = 0;
#pragma unroll
    for (int i = 0; i < 6 * NP; ++i) P[i] = r.blk(i);
#pragma unroll
    for (int i = 0; i < 3 * NA; ++i) P[6 * NP + i] = r.blk(6 * M15::NP + i);
    DetV<T> fmax = run;
    if (a.root_mask) {
        const DetBand<T> band(a);
        for (uint64_t rest = a.root_mask; rest; rest &= rest - 1) {
            RegSink<T, NR> sk;
            sk.on = true;
            uint64_t b0 = 0, c0 = 0, b1 = 0, c1 = 0;
            // j = the candidate's index relative to the free ones (negative: a.ev + 11 j is the
            // fixed event's row of a.ev_all)
            search_child_to<T, CUSTOM, SYM, ParRegs<T>, RegSink<T, NR>, false>(
                a, band, *this, ParRegs<T>{P}, __builtin_ctzll(rest) - a.shift, sk, false, b0, c0, b1, c1);
#pragma unroll
            for (int i = 0; i < NR; ++i) P[i] = sk.P[i];
            run = sk.run;
            prev = sk.prev;
            mask = sk.mask;
            fmax = sk.fmax;
        }
    }
    (void)eval;
    return fmax;
}

template <typename T, bool CUSTOM, bool SYM, class PS>
__device__ __forceinline__ void search_child(const Ref15SearchArgs& a, const DetBand<T>& band,
                                             const SearchNode<T, CUSTOM, SYM>& par, const PS& pp, int j, uint64_t c,
                                             uint64_t& best, uint64_t& cnt, uint64_t& best1, uint64_t& cnt1) {
    const bool store = a.child && j < a.n_events - 2;
    LevelSink<T, SYM> sk{store ? level_block<T, SYM>(a.child, c) : nullptr, uint32_t(c) & 63u, store};
    search_child_to<T, CUSTOM, SYM>(a, band, par, pp, j, sk, a.tail && j == a.n_events - 2,  // wave-uniform (j is)
                                    best, cnt, best1, cnt1);
}

// one atomic pair per wave, and only from waves with an accepted subset; k = local level
__device__ __forceinline__ void search_publish(const Ref15SearchArgs& a, int k, uint64_t best, uint64_t cnt) {
    if (__builtin_amdgcn_ballot_w64(cnt != 0) != 0) {  // wave-uniform
        best = wave_max_u64(best);
        cnt = wave_sum_u64(cnt);
        if (__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) == 0) {
            atomicMax(reinterpret_cast<unsigned long long*>(&a.best[a.k_base + k]), static_cast<unsigned long long>(best));
            atomicAdd(reinterpret_cast<unsigned long long*>(&a.n_acc[a.k_base + k]), static_cast<unsigned long long>(cnt));
        }
    }
}

// Parent-major: one lane per parent, its children in a wave-uniform loop over j (parents of a
// wave share their largest event except at run boundaries, so event j is the same for every
// active lane: scalar loads, a uniform GPS/IMU branch).  For the wide levels.
#ifndef KF_SEARCH_PM_WAVES
#define KF_SEARCH_PM_WAVES 2  // waves per SIMD of the register variant (its VGPR budget)
#endif
// Ref15SearchArgs::stop_best: lane i reads size stop_lo + i (vector loads: these counters were
// written by earlier launches' atomics); the same answer in every wave of the grid.  Called
// before any lane leaves the kernel.
__device__ __forceinline__ bool search_stopped(const Ref15SearchArgs& a) {
    if (!a.stop_best) return false;
    const int s = a.stop_lo + int(threadIdx.x & 63u);
    const uint64_t v = s <= a.stop_hi ? __atomic_load_n(a.stop_best + s, __ATOMIC_RELAXED) : 0;
    return __any(v != 0);
}

#ifndef KF_SEARCH_SYM_WAVES
#define KF_SEARCH_SYM_WAVES 3  // waves per SIMD of the axis-symmetric search kernels (A/B builds)
#endif
// PLDS: the parent's covariance lives in LDS (one 64-lane block per workgroup, [27][64] T),
// which fits the kernel in 3 waves per SIMD without spills; otherwise in registers.
template <typename T, bool PLDS, bool CUSTOM, bool SYM>
__global__ __launch_bounds__(PLDS ? 64 : kBlock) __attribute__((
    amdgpu_waves_per_eu(SYM ? KF_SEARCH_SYM_WAVES : PLDS ? 3 : KF_SEARCH_PM_WAVES))) void
ref15_search_pm_kernel(const Ref15SearchArgs a) {
    if (search_stopped(a)) return;
    constexpr int NT = PLDS ? 64 : kBlock;
    constexpr int NR = SearchNode<T, CUSTOM, SYM>::NR;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * NT + threadIdx.x;
    if (uint64_t(p) >= a.n_par) return;
    const DetBand<T> band(a);
    SearchNode<T, CUSTOM, SYM> par;
    if (a.k == 1) {
        uint64_t rb = 0, rc = 0;  // a fixed root is itself one of the subsets searched
        const DetV<T> f = par.root(a, a.root_mask != 0);
        if (a.root_mask) search_score(a, band, a.root_mask, f, rb, rc);
        search_publish(a, 0, rb, rc);
    } else {
        par.load(a.par, uint64_t(p));
    }
    const int m = par.max_event(a.shift);
    const int j0 = wave_uniform(m) + 1;  // colex order: the first lane holds the smallest max
    uint64_t best = 0, cnt = 0, best1 = 0, cnt1 = 0;
    if constexpr (PLDS) {
        __shared__ T sP[NR * 64];
        T* col = sP + threadIdx.x;
#pragma unroll
        for (int i = 0; i < NR; ++i) col[i * 64] = par.P[i];  // read back by this lane only
        const ParLds<T> pp{col};
#pragma unroll 1
        for (int j = j0; j < a.n_events; ++j) {
            if (j <= m) continue;
            search_child<T, CUSTOM, SYM>(a, band, par, pp, j, uint64_t(p) + ro(a.binom)[j * (kMaxEvents + 1) + a.k], best,
                                         cnt, best1, cnt1);
        }
    } else {
        const ParRegs<T> pp{par.P};
#pragma unroll 1
        for (int j = j0; j < a.n_events; ++j) {
            if (j <= m) continue;
            search_child<T, CUSTOM, SYM>(a, band, par, pp, j, uint64_t(p) + ro(a.binom)[j * (kMaxEvents + 1) + a.k], best,
                                         cnt, best1, cnt1);
        }
    }
    search_publish(a, a.k, best, cnt);
    if (a.tail) search_publish(a, a.k + 1, best1, cnt1);
}

// Two levels per launch (KF_OPT_SEARCH_PAIR, the axis-symmetric search's parent-major levels):
// lane p's parent (level k - 1, stored), each of its children (level k) computed into the lane's
// LDS column — not stored — and, at once, that child's children (level k + 1) from the column,
// stored as the next launch's parents.  Each subset's operations are search_child's and a child
// reaches its children with the bits a stored node would carry, so every score and every stored
// node is the one-level search's; level k's nodes (half the level traffic) never reach HBM.  A
// child holding event n - 2 has one child (it plus n - 1), scored by its tail as size k + 1.
template <typename T, bool CUSTOM, bool SYM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(KF_SEARCH_SYM_WAVES))) void
ref15_search_pair_kernel(const Ref15SearchArgs a) {
    if (search_stopped(a)) return;
    constexpr int NR = SearchNode<T, CUSTOM, SYM>::NR;
    const int64_t p = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
    if (uint64_t(p) >= a.n_par) return;
    const int n = a.n_events, k = a.k;
    const DetBand<T> band(a);
    SearchNode<T, CUSTOM, SYM> par;
    par.load(a.par, uint64_t(p));
    const int m = par.max_event(a.shift);
    const int j0 = wave_uniform(m) + 1;  // colex order: the first lane holds the smallest max
    __shared__ T sP[NR * 64];
    __shared__ T sC[NR * 64];
    T* col = sP + threadIdx.x;
    T* ccol = sC + threadIdx.x;
#pragma unroll
    for (int i = 0; i < NR; ++i) col[i * 64] = par.P[i];  // read back by this lane only
    const ParLds<T> pp{col}, cp{ccol};
    uint64_t best = 0, cnt = 0, best1 = 0, cnt1 = 0, best2 = 0, cnt2 = 0;
#pragma unroll 1
    for (int j = j0; j < n; ++j) {
        if (j <= m) continue;
        LdsSink<T> sk{ccol, j < n - 2};
        search_child_to<T, CUSTOM, SYM>(a, band, par, pp, j, sk, j == n - 2, best, cnt, best1, cnt1);
        if (j < n - 2) {  // wave-uniform
            SearchNode<T, CUSTOM, SYM> ch;
            ch.run = sk.run;
            ch.prev = sk.prev;
            ch.mask = sk.mask;
            const uint64_t c = uint64_t(p) + ro(a.binom)[j * (kMaxEvents + 1) + k];  // the child's rank at level k
#pragma unroll 1
            for (int j2 = j + 1; j2 < n; ++j2)
                search_child<T, CUSTOM, SYM>(a, band, ch, cp, j2, c + ro(a.binom)[j2 * (kMaxEvents + 1) + k + 1], best1,
                                             cnt1, best2, cnt2);
        }
    }
    search_publish(a, k, best, cnt);
    search_publish(a, k + 1, best1, cnt1);
    if (a.tail) search_publish(a, k + 2, best2, cnt2);
}

// The head of the search: levels 1 .. K (a.k = K) in ONE launch, one lane per subset of at most
// K free candidates — lanes in (size, colex rank) order — each run from the root through its
// events in index order with the level kernels' per-chain operations, so every score and every
// stored node is the level search's, bit for bit.  It replaces K launches whose first few hold a
// few dozen to a few thousand subsets each and sit at a launch-and-one-event floor of ~10 us
// (DESIGN.md §3).  Level K's subsets whose largest candidate is <= n - 3 are stored as level
// K + 1's parents; one whose largest is n - 2 also scores its child with n - 1 (the tail).
// a.n_child = sum_{k <= K} C(n, k).  Every lane stays to the end (the publish reductions read
// every lane).
// The binomials C(x, y), x <= n, y <= ymax, of the one-lane-per-subset kernels (head, end) in
// LDS: their colex unranking walks up to n candidates per lane, each step a binomial load that
// the next step depends on, so each step waits an LDS latency instead of an L1/L2 one.
// Dynamic LDS of search_binom_lds_bytes(n, ymax); every lane of the block calls it.
__host__ __device__ constexpr size_t search_binom_lds_bytes(int n, int ymax) {
    return sizeof(uint64_t) * size_t(n + 1) * size_t(ymax + 1);
}
__device__ __forceinline__ const uint64_t* search_binom_lds(const Ref15SearchArgs& a, int ymax) {
    extern __shared__ uint64_t sbinom[];
    const int n = a.n_events, w = ymax + 1, tot = (n + 1) * w;
    for (int i = int(threadIdx.x); i < tot; i += int(blockDim.x)) {
        const int x = i / w, y = i - x * w;
        sbinom[i] = a.binom[x * (kMaxEvents + 1) + y];
    }
    __syncthreads();
    return sbinom;
}

// The body shared by the head launch (one search) and the many-window launch (one search per
// blockIdx.y): the one-wave workgroup's lanes are subsets blockIdx.x * 64 + lane of search `a`.
template <typename T, bool CUSTOM, bool SYM>
__device__ __forceinline__ void search_head_lanes(const Ref15SearchArgs& a) {
    using Node = SearchNode<T, CUSTOM, SYM>;
    constexpr int RP = SYM ? M15::NP : 1, RA = SYM ? M15::NA : 1;
    const int n = a.n_events, K = a.k;
    const uint64_t* C = search_binom_lds(a, K + 1);  // C(n, k) for k <= K, C(c, i) for i <= K
    auto binom = [&](int x, int y) -> uint64_t { return C[x * (K + 2) + y]; };
    const uint64_t g = uint64_t(blockIdx.x) * 64 + threadIdx.x;
    const bool live = g < a.n_child;
    int k = 1;
    uint64_t r = live ? g : 0;
    while (k < K && r >= binom(n, k)) {
        r -= binom(n, k);
        ++k;
    }
    // colex unranking: rank r = sum_i C(c_i, i) over the sorted members c_1 < ... < c_k
    uint64_t sub = 0;
    {
        uint64_t rr = r;
        int c = n - 1;
        for (int i = k; i >= 1; --i) {
            while (binom(c, i) > rr) --c;
            rr -= binom(c, i);
            sub |= uint64_t(1) << c;
            --c;
        }
    }
    uint64_t best = 0, cnt = 0, best1 = 0, cnt1 = 0;
    const DetBand<T> band(a);
    Node nd;
    {
        uint64_t rb = 0, rc = 0;  // a fixed root is itself one of the subsets searched (lane 0 scores it)
        const bool eval = a.root_mask != 0 && g == 0;
        const DetV<T> f = nd.root(a, eval);
        if (eval) search_score(a, band, a.root_mask, f, rb, rc);
        search_publish(a, 0, rb, rc);
    }
    DetV<T> fmax = nd.run;
#pragma unroll 1
    for (uint64_t m = sub; m; m &= m - 1) {
        const int j = __builtin_ctzll(m);
        SearchEvent vs = search_event(a, j, nd.prev);
        vs.final_predict = vs.final_predict && (m & (m - 1)) == 0;  // only the subset itself is scored
        SearchScore<T, CUSTOM> ss;
        ss.kc = a.kc;
#pragma unroll
        for (int ch = 0; ch < Node::NP; ++ch) {
            T Pb[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) Pb[i] = nd.P[6 * ch + i];
            search_pva<T, CUSTOM>(vs, ch, Pb, ss.ok, a.kc);
#pragma unroll
            for (int i = 0; i < 6; ++i) nd.P[6 * ch + i] = Pb[i];
            ss.add_pva(vs, Pb, ch, RP);
        }
#pragma unroll
        for (int ch = 0; ch < Node::NA; ++ch) {
            T Pa[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) Pa[i] = nd.P[6 * Node::NP + 3 * ch + i];
            search_aw<T, CUSTOM>(vs, ch, Pa, ss.ok, a.kc);
#pragma unroll
            for (int i = 0; i < 3; ++i) nd.P[6 * Node::NP + 3 * ch + i] = Pa[i];
            ss.add_aw(vs, Pa, ch, RA);
        }
        nd.run = ss.finish(vs, nd.run, fmax);
        nd.prev = vs.prev;
        nd.mask |= uint64_t(1) << (j + a.shift);
    }
    const int top = sub ? 63 - __builtin_clzll(sub) : -1;
    if (live) {
        search_score(a, band, nd.mask, fmax, best, cnt);
        if (k == K && a.child && top <= n - 3) nd.store(a.child, r);  // level K + 1's parent, at its colex rank
        if (k == K && a.tail && top == n - 2) {  // its only child, plus event n - 1 (size K + 1)
            const SearchEvent vg = search_event(a, n - 1, nd.prev);
            SearchScore<T, CUSTOM> sg;
            sg.kc = a.kc;
#pragma unroll
            for (int ch = 0; ch < Node::NP; ++ch) {
                T Pb[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) Pb[i] = nd.P[6 * ch + i];
                search_pva<T, CUSTOM>(vg, ch, Pb, sg.ok, a.kc);
                sg.add_pva(vg, Pb, ch, RP);
            }
#pragma unroll
            for (int ch = 0; ch < Node::NA; ++ch) {
                T Pa[3];
#pragma unroll
                for (int i = 0; i < 3; ++i) Pa[i] = nd.P[6 * Node::NP + 3 * ch + i];
                search_aw<T, CUSTOM>(vg, ch, Pa, sg.ok, a.kc);
                sg.add_aw(vg, Pa, ch, RA);
            }
            DetV<T> gmax;
            (void)sg.finish(vg, nd.run, gmax);
            search_score(a, band, nd.mask | (uint64_t(1) << (n - 1 + a.shift)), gmax, best1, cnt1);
        }
    }
    // per size: a wave holds lanes of at most a few consecutive sizes
#pragma unroll 1
    for (int kk = 1; kk <= K; ++kk)
        if (__builtin_amdgcn_ballot_w64(live && k == kk) != 0)
            search_publish(a, kk, k == kk ? best : 0, k == kk ? cnt : 0);
    if (a.tail) search_publish(a, K + 1, best1, cnt1);
}

template <typename T, bool CUSTOM, bool SYM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SYM ? KF_SEARCH_SYM_WAVES : 3))) void ref15_search_head_kernel(
    const Ref15SearchArgs a) {
    search_head_lanes<T, CUSTOM, SYM>(a);
}

// Many windows in one launch (kf_search_windows): workgroup (x, w) is wave x of window w's
// search, sizes 1 .. wins[w].k with nothing fixed and nothing stored — the head launch's lanes for
// that window, so every score is kf_search_combos'.  The window's arguments are read through the
// constant address space by the wave-uniform blockIdx.y (scalar loads).  A workgroup past its
// window's lanes leaves whole, ahead of the binomial fill's barrier.  Dynamic LDS: the binomials
// of the widest (n, k) of the call.
template <typename T, bool CUSTOM, bool SYM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SYM ? KF_SEARCH_SYM_WAVES : 3))) void ref15_search_windows_kernel(
    const Ref15WindowArgs* wins, const uint64_t* binom, const RefConsts* kc) {
    const auto* w = ro(wins) + blockIdx.y;
    if (uint64_t(blockIdx.x) * 64 >= w->n_child) return;
    Ref15SearchArgs a;
    a.n_events = w->n_events;
    a.k = w->k;
    a.shift = 0;
    a.k_base = 0;
    a.root_mask = 0;
    a.ev_all = a.ev = w->ev;
    a.n_child = w->n_child;
    a.binom = binom;
    a.init = w->init;
    a.prev_time = w->prev_time;
    a.target_end = w->target_end;
    a.threshold = w->threshold;
    a.band_lo_m = w->band_lo_m;
    a.band_hi_m = w->band_hi_m;
    a.band_lo_e = w->band_lo_e;
    a.band_hi_e = w->band_hi_e;
    a.band_mode = w->band_mode;
    a.child = nullptr;
    a.best = w->best;
    a.n_acc = w->n_acc;
    a.subset_max = nullptr;
    a.tail = 0;
    a.kc = kc;
    search_head_lanes<T, CUSTOM, SYM>(a);
}

// kf_search_windows' results: thread w turns window w's counters into (winner, k_found,
// n_accepted[0 .. k_max]) in the mapped host buffer, by kf_search_combos' rule for a search that
// stops at the first accepted size (the call clears the counters before its launch).
__global__ __launch_bounds__(256) void search_windows_finish_kernel(const Ref15WindowArgs* wins, int W, int k_max,
                                                                    uint64_t* host) {
    const int w = int(blockIdx.x) * 256 + int(threadIdx.x);
    if (w < W) {
        const uint64_t* best = wins[w].best;
        const uint64_t* acc = wins[w].n_acc;
        const int k = wins[w].k;
        int found = 0;
        for (int i = 1; i <= k && !found; ++i)
            if (best[i]) found = i;
        uint64_t* out = host + int64_t(w) * (3 + k_max);
        out[0] = found ? __builtin_bitreverse64(best[found]) : 0;
        out[1] = uint64_t(found);
        for (int i = 0; i <= k_max; ++i) out[2 + i] = found && i <= found ? acc[i] : 0;
    }
    __threadfence_system();
}

// The end of the search, sizes a.k .. a.k_end (free sizes) in ONE launch, extension-major: a
// subset S of size >= a.k is its (a.k - 1)-prefix P (its smallest members, a node of level
// a.k - 1) plus its extension E (the rest).  For an extension E whose smallest member is e, the
// prefixes are every (a.k - 1)-subset of 0 .. e - 1, which are level a.k - 1's colex ranks
// 0 .. C(e, a.k - 1) - 1, all stored (their largest member is <= n - 3) except, for E = {n - 1},
// the ranks from C(n - 2, a.k - 1) on, whose subsets level a.k - 1's tail scored.  So one wave
// takes one extension and 64 consecutive prefixes: its node loads are one parent block, its
// events and subset size are wave-uniform, and nothing is unranked.  Group i of the host's table
// is extension gblk[i] (a mask of free candidates, ordered by size), its waves start at
// gitem[i].  Every subset's score is the level search's, bit for bit (the level kernels' per-chain
// operations from the same stored node).  It replaces the last levels' launches, which hold a few
// thousand subsets or fewer and sit at the launch-and-one-event floor.
template <typename T, bool CUSTOM, bool SYM>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SYM ? KF_SEARCH_SYM_WAVES : 3))) void ref15_search_end_kernel(
    const Ref15SearchArgs a) {
    if (search_stopped(a)) return;
    using Node = SearchNode<T, CUSTOM, SYM>;
    constexpr int RP = SYM ? M15::NP : 1, RA = SYM ? M15::NA : 1;
    const int n = a.n_events, K0 = a.k;
    const uint64_t w = blockIdx.x;
    int lo = 0, hi = a.n_groups - 1;  // the last group whose first wave is <= w
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.gitem[mid] <= w) lo = mid;
        else hi = mid - 1;
    }
    const uint64_t ext = a.gblk[lo];
    const int e = __builtin_ctzll(ext);
    const int ex = e == n - 1 ? n - 2 : e;  // E = {n - 1}: the stored prefixes only
    const uint64_t n_pre = ro(a.binom)[ex * (kMaxEvents + 1) + K0 - 1];
    const uint64_t rp = (w - a.gitem[lo]) * 64 + threadIdx.x;
    const bool live = rp < n_pre;
    uint64_t best = 0, cnt = 0;
    const DetBand<T> band(a);
    Node nd;
    nd.load(a.par, live ? rp : 0);  // a stored node either way (rank 0 is)
    DetV<T> fmax = nd.run;
#pragma unroll 1
    for (uint64_t m = ext; m; m &= m - 1) {
        const int j = __builtin_ctzll(m);
        SearchEvent vs = search_event(a, j, nd.prev);
        vs.final_predict = vs.final_predict && (m & (m - 1)) == 0;  // only the subset itself is scored
        SearchScore<T, CUSTOM> ss;
        ss.kc = a.kc;
#pragma unroll
        for (int ch = 0; ch < Node::NP; ++ch) {
            T Pb[6];
#pragma unroll
            for (int i = 0; i < 6; ++i) Pb[i] = nd.P[6 * ch + i];
            search_pva<T, CUSTOM>(vs, ch, Pb, ss.ok, a.kc);
#pragma unroll
            for (int i = 0; i < 6; ++i) nd.P[6 * ch + i] = Pb[i];
            ss.add_pva(vs, Pb, ch, RP);
        }
#pragma unroll
        for (int ch = 0; ch < Node::NA; ++ch) {
            T Pa[3];
#pragma unroll
            for (int i = 0; i < 3; ++i) Pa[i] = nd.P[6 * Node::NP + 3 * ch + i];
            search_aw<T, CUSTOM>(vs, ch, Pa, ss.ok, a.kc);
#pragma unroll
            for (int i = 0; i < 3; ++i) nd.P[6 * Node::NP + 3 * ch + i] = Pa[i];
            ss.add_aw(vs, Pa, ch, RA);
        }
        nd.run = ss.finish(vs, nd.run, fmax);
        nd.prev = vs.prev;
        nd.mask |= uint64_t(1) << (j + a.shift);
    }
    if (live) search_score(a, band, nd.mask, fmax, best, cnt);
    search_publish(a, K0 - 1 + __builtin_popcountll(ext), best, cnt);
}

// Child-major: one wave per (parent block of 64, child event) work item, one child per lane,
// so no lane walks a long list of children (the narrow levels, where few parents have many
// children each).  Items are ordered by parent block, then j, and dealt to the XCDs in
// contiguous ranges, so the items that read one parent block run back to back on one XCD and
// re-read it from that XCD's L2.  Blocks are grouped by their first parent's largest event v
// (non-decreasing in colex order); a block of group v has items j = v + 1 .. n - 1.
// PAIR (the axis-symmetric search, KF_OPT_SEARCH_PAIR): levels k and k + 1 in one launch — each
// lane's child j (level k) computed into its LDS column, never stored, then that child's children
// j2 > j (level k + 1) from the column, stored as the next launch's parents, as the parent-major
// pair kernel does; the items keep this kernel's parallelism (a parent block per child event).
template <typename T, bool CUSTOM, bool SYM, bool PAIR = false>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(SYM ? KF_SEARCH_SYM_WAVES : 3))) void ref15_search_cm_kernel(const Ref15SearchArgs a,
                                                                                                     uint64_t n_items) {
    if (search_stopped(a)) return;
    const uint64_t per_xcd = (n_items + 7) / 8;
    const uint64_t item = uint64_t(blockIdx.x % 8) * per_xcd + blockIdx.x / 8;
    if (item >= n_items) return;
    const int n = a.n_events, k = a.k;
    ro_u64* C = ro(a.binom);
    auto binom = [&](int x, int y) -> uint64_t { return x < 0 ? (y == 0 ? 1 : 0) : C[x * (kMaxEvents + 1) + y]; };
    // the item's group (the host's table in the kernel arguments: a binary search over
    // constant-cache loads, instead of a walk whose every step waited on a binomial load)
    int v = -1;
    uint64_t blk = 0;
    int j = int(item);  // k == 1: item j is the root's child j
    if (k > 1) {
        int lo = 0, hi = a.n_groups - 1;  // the last group whose first item is <= item
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (a.gitem[mid] <= item) lo = mid;
            else hi = mid - 1;
        }
        v = a.v_lo + lo;
        const uint32_t r = uint32_t(item - a.gitem[lo]), w = uint32_t(n - 1 - v);  // r < 2^31 (host check)
        const uint32_t q = r / w;
        blk = a.gblk[lo] + q;
        j = v + 1 + int(r - q * w);
    }
    const uint64_t p = blk * 64 + threadIdx.x;
    if (p >= a.n_par) return;
    const DetBand<T> band(a);
    SearchNode<T, CUSTOM, SYM> par;
    if (k == 1) {
        uint64_t rb = 0, rc = 0;  // a fixed root is itself one of the subsets searched (item 0 scores it)
        const bool eval = a.root_mask != 0 && item == 0;
        const DetV<T> f = par.root(a, eval);
        if (eval) search_score(a, band, a.root_mask, f, rb, rc);
        search_publish(a, 0, rb, rc);
    } else {
        par.load(a.par, p);
    }
    uint64_t best = 0, cnt = 0, best1 = 0, cnt1 = 0;
    if constexpr (PAIR) {
        constexpr int NR = SearchNode<T, CUSTOM, SYM>::NR;
        __shared__ T sC[NR * 64];
        T* ccol = sC + threadIdx.x;
        uint64_t best2 = 0, cnt2 = 0;
        if (par.max_event(a.shift) < j) {
            LdsSink<T> sk{ccol, j < n - 2};
            // a child holding n - 2 has the one child adding n - 1: its tail, size k + 1
            search_child_to<T, CUSTOM, SYM>(a, band, par, ParRegs<T>{par.P}, j, sk, j == n - 2, best, cnt, best1, cnt1);
            if (j < n - 2) {  // wave-uniform (j is)
                SearchNode<T, CUSTOM, SYM> ch;
                ch.run = sk.run;
                ch.prev = sk.prev;
                ch.mask = sk.mask;
                const uint64_t c = p + binom(j, k);  // the child's rank at level k
#pragma unroll 1
                for (int j2 = j + 1; j2 < n; ++j2)
                    search_child<T, CUSTOM, SYM>(a, band, ch, ParLds<T>{ccol}, j2, c + binom(j2, k + 1), best1, cnt1,
                                                 best2, cnt2);
            }
        }
        search_publish(a, k, best, cnt);
        search_publish(a, k + 1, best1, cnt1);
        if (a.tail) search_publish(a, k + 2, best2, cnt2);
    } else {
        if (par.max_event(a.shift) < j)
            search_child<T, CUSTOM, SYM>(a, band, par, ParRegs<T>{par.P}, j, p + binom(j, k), best, cnt, best1, cnt1);
        search_publish(a, a.k, best, cnt);
        if (a.tail) search_publish(a, a.k + 1, best1, cnt1);
    }
}

// kf_search_combos' counters (best[], n_acc[]) to the handle's mapped host buffer (vector
// stores, made visible to the host before the kernel ends): after a level of a non-exhaustive
// search (peek), and at the end, where they are also zeroed for the next search on the stream.
__global__ __launch_bounds__(256) void search_finish_kernel(uint64_t* counters, uint64_t* host, int n, bool zero) {
    const int i = int(threadIdx.x);
    if (i < n) {
        host[i] = counters[i];
        if (zero) counters[i] = 0;
    }
    __threadfence_system();
}
}  // namespace

hipError_t launch_ref15_combos(bool f64, const Ref15ComboArgs& a, hipStream_t stream) {
    if (a.n_events > kMaxEvents) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>((a.B + kBlock - 1) / kBlock));
    KF_CUSTOM_DISPATCH(a.kc, KF_DTYPE_DISPATCH(f64, ref15_combo_kernel<T, CUSTOM><<<grid, kBlock, 0, stream>>>(a)));
    return hipGetLastError();
}

void set_search_band(Ref15SearchArgs& a, bool f64) {
    // the threshold as the kernels compare it (T(threshold)); (mantissa, exponent) pairs whose
    // mantissa T's rounding keeps far inside eps (a mantissa rounded up to 1 only makes the
    // kernels' (e, m) comparisons conservative)
    // |log det| of a 15 x 15 SPD matrix stays below 15 * 745 (every pivot is a finite double, a
    // float's log below 15 * 104): above 1e5 the test accepts every valid determinant; below
    // -1e5 only one that underflowed to 0 (its log is -inf), and none at -inf or NaN
    const double t = f64 ? a.threshold : double(float(a.threshold));
    a.band_mode = t == t ? (t > 1e5 ? 1 : (t < -1e5 ? (t == -HUGE_VAL ? 3 : 2) : 0)) : 3;
    a.band_lo_m = a.band_hi_m = 1.0;
    a.band_lo_e = a.band_hi_e = 0;
    if (a.band_mode != 0) return;
    // the band's half-width in log units: above the log's absolute rounding near t (a few ulps of
    // t in T) and this exp2's (q - fl carries q's rounding, 1e-16 |t|)
    const double eps = f64 ? std::fmax(1e-10, std::fabs(t) * 1e-14) : std::fmax(1e-4, std::fabs(t) * 1e-6);
    const double q = t * 1.4426950408889634074;  // thr / ln 2: e^thr = 2^fl * 2^(q - fl)
    const double fl = std::floor(q);
    const double mm = std::exp2(q - fl);
    int e1, e2;
    a.band_lo_m = std::frexp(mm * (1.0 - eps), &e1);
    a.band_hi_m = std::frexp(mm * (1.0 + eps), &e2);
    a.band_lo_e = int(fl) + e1;
    a.band_hi_e = int(fl) + e2;
}

hipError_t launch_search_finish(uint64_t* counters, uint64_t* host, int n, bool zero, hipStream_t stream) {
    if (n < 1 || n > 256) return hipErrorInvalidValue;
    search_finish_kernel<<<1, 256, 0, stream>>>(counters, host, n, zero);
    return hipGetLastError();
}

hipError_t launch_ref15_search_end(bool f64, const Ref15SearchArgs& a, hipStream_t stream) {
    if (a.n_events > kMaxEvents || a.k < 2 || a.k_end < a.k || a.k_end > a.n_events || !a.par || a.n_groups < 1 ||
        a.n_groups > 65 || a.gitem[a.n_groups] == 0 || a.gitem[a.n_groups] >= (1ull << 31))
        return hipErrorInvalidValue;
    // the extensions' table (group i: extension gblk[i], first wave gitem[i], then the total)
    const dim3 grid(unsigned(a.gitem[a.n_groups]));
    KF_CUSTOM_DISPATCH(a.kc, KF_BOOL_DISPATCH(a.sym, SYM, KF_DTYPE_DISPATCH(f64,
        ref15_search_end_kernel<T, CUSTOM, SYM><<<grid, 64, 0, stream>>>(a))));
    return hipGetLastError();
}

hipError_t launch_ref15_search_windows(bool f64, bool sym, const Ref15WindowArgs* wins, int W, uint64_t max_lanes,
                                       int n_max, int k_max, const uint64_t* binom, const RefConsts* kc,
                                       hipStream_t stream) {
    if (W < 1 || W > 65535 || n_max < 1 || n_max > kMaxEvents || k_max < 1 || k_max > kSearchWindowsMaxK ||
        max_lanes == 0 || max_lanes * uint64_t(W) >= (1ull << 31))  // kf_search_windows' documented limit
        return hipErrorInvalidValue;
    const dim3 grid(unsigned((max_lanes + 63) / 64), unsigned(W));
    const size_t lds = search_binom_lds_bytes(n_max, k_max + 1);
    KF_CUSTOM_DISPATCH(kc, KF_BOOL_DISPATCH(sym, SYM, KF_DTYPE_DISPATCH(f64,
        ref15_search_windows_kernel<T, CUSTOM, SYM><<<grid, 64, lds, stream>>>(wins, binom, kc))));
    return hipGetLastError();
}

hipError_t launch_search_windows_finish(const Ref15WindowArgs* wins, int W, int k_max, uint64_t* host,
                                        hipStream_t stream) {
    if (W < 1 || k_max < 1 || k_max > kSearchWindowsMaxK) return hipErrorInvalidValue;
    search_windows_finish_kernel<<<dim3(unsigned((W + 255) / 256)), 256, 0, stream>>>(wins, W, k_max, host);
    return hipGetLastError();
}

hipError_t launch_ref15_search_head(bool f64, const Ref15SearchArgs& a, hipStream_t stream) {
    if (a.n_events > kMaxEvents || a.n_events < 3 || a.k < 1 || a.k > a.n_events - 2 || a.n_child == 0 ||
        a.n_child >= (1ull << 31))
        return hipErrorInvalidValue;
    const dim3 grid(unsigned((a.n_child + 63) / 64));
    const size_t lds = search_binom_lds_bytes(a.n_events, a.k + 1);
    KF_CUSTOM_DISPATCH(a.kc, KF_BOOL_DISPATCH(a.sym, SYM, KF_DTYPE_DISPATCH(f64,
        ref15_search_head_kernel<T, CUSTOM, SYM><<<grid, 64, lds, stream>>>(a))));
    return hipGetLastError();
}

// The child-major kernel's work items: per group v of parent blocks, blocks x (n - 1 - v) child
// events; group v holds blocks [ceil(C(v, k-1)/64), ceil(C(v+1, k-1)/64)) (the stored parents
// have largest event <= n - 3).  Fills b's group table; false when the items overflow.
static bool cm_items(const Ref15SearchArgs& a, Ref15SearchArgs& b, uint64_t& items, uint64_t& waves) {
    const uint64_t* C = a.binom_host;
    const int n = a.n_events, k = a.k;
    b = a;
    items = 0;
    if (k == 1) {
        items = uint64_t(n);
        b.n_groups = 0;
    } else {
        b.v_lo = k - 2;
        int i = 0;
        for (int v = k - 2; v <= n - 3; ++v, ++i) {
            const uint64_t b0 = (C[v * (kMaxEvents + 1) + k - 1] + 63) / 64;
            const uint64_t b1 = (C[(v + 1) * (kMaxEvents + 1) + k - 1] + 63) / 64;
            b.gitem[i] = items;
            b.gblk[i] = b0;
            const uint64_t span = (b1 - b0) * uint64_t(n - 1 - v);
            if (span >= (1ull << 31)) return false;  // 32-bit item offsets in a group
            items += span;
        }
        b.n_groups = i;
        if (i == 0) return false;
    }
    waves = (items + 7) / 8 * 8;
    return waves < (1ull << 31);
}

hipError_t launch_ref15_search(bool f64, const Ref15SearchArgs& a, bool child_major, hipStream_t stream) {
    // the stored parents (kf_search_combos' cap); a level's children C(n, k) may be many more
    // (n = 40, k = 10: 8.5e8): child ranks and node addresses are 64-bit, and only the children
    // below C(n - 2, k) are stored
    if (a.n_events > kMaxEvents || a.k < 1 || a.k > a.n_events || a.n_par == 0 || a.n_par >= (1ull << 28))
        return hipErrorInvalidValue;
    if (child_major) {
        Ref15SearchArgs b;
        uint64_t items = 0, waves = 0;
        if (!cm_items(a, b, items, waves)) return hipErrorInvalidValue;
        KF_CUSTOM_DISPATCH(a.kc, KF_BOOL_DISPATCH(a.sym, SYM, KF_DTYPE_DISPATCH(f64,
            ref15_search_cm_kernel<T, CUSTOM, SYM><<<dim3(unsigned(waves)), 64, 0, stream>>>(b, items))));
        return hipGetLastError();
    }
    // PLDS: the parents' covariances in LDS, one wave per workgroup; otherwise (a.pm_regs) in registers
    KF_CUSTOM_DISPATCH(a.kc, KF_BOOL_DISPATCH(!a.pm_regs, PLDS, KF_BOOL_DISPATCH(a.sym, SYM, KF_DTYPE_DISPATCH(f64, {
        constexpr unsigned block = PLDS ? 64 : kBlock;
        const dim3 grid(static_cast<unsigned>((a.n_par + block - 1) / block));
        ref15_search_pm_kernel<T, PLDS, CUSTOM, SYM><<<grid, block, 0, stream>>>(a);
    }))));
    return hipGetLastError();
}

hipError_t launch_ref15_search_pair(bool f64, const Ref15SearchArgs& a, bool child_major, hipStream_t stream) {
    // levels k and k + 1 <= n of the axis-symmetric search, from level k - 1's stored parents
    if (!a.sym || a.n_events > kMaxEvents || a.k < 2 || a.k + 1 > a.n_events || a.n_par == 0 ||
        a.n_par >= (1ull << 28) || !a.par)
        return hipErrorInvalidValue;
    if (child_major) {
        Ref15SearchArgs b;
        uint64_t items = 0, waves = 0;
        if (!cm_items(a, b, items, waves)) return hipErrorInvalidValue;
        KF_CUSTOM_DISPATCH(a.kc, KF_DTYPE_DISPATCH(f64,
            ref15_search_cm_kernel<T, CUSTOM, true, true><<<dim3(unsigned(waves)), 64, 0, stream>>>(b, items)));
        return hipGetLastError();
    }
    const dim3 grid(static_cast<unsigned>((a.n_par + 63) / 64));
    KF_CUSTOM_DISPATCH(a.kc, KF_DTYPE_DISPATCH(f64, ref15_search_pair_kernel<T, CUSTOM, true><<<grid, 64, 0, stream>>>(a)));
    return hipGetLastError();
}

}  // namespace kfmi

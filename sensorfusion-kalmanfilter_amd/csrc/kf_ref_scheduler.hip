// The scheduler of the 15-state model (kf_ref_model.h): scoring a candidate update
// (kf_score_*: launch_ref15_score), random picks (kf_sched_random_picks:
// launch_ref15_random_picks) and the rate-decimated greedy run (kf_run_scheduled*:
// launch_ref15_scheduled), fused in one kernel or as a pick pass and an apply pass.  The waves are
// ordered by pick-list length with sort_pairs_desc_u32 (kf_sort.hip).
#include "kf_ref_model.h"

namespace kfmi {
namespace {

// ------------------------------------------------------------------------------------
// Scheduler scoring and the rate-decimated greedy driver (kf_workers.py:99-213, 826-957).
// ------------------------------------------------------------------------------------
template <typename T, bool CUSTOM>
__device__ __forceinline__ T cov_trace(const Ref15<T, CUSTOM>& s) {
    T tr = T(0);
#pragma unroll
    for (int i = 0; i < 3; ++i) tr += s.pva[i][0] + s.pva[i][3] + s.pva[i][5];
#pragma unroll
    for (int i = 0; i < 3; ++i) tr += s.aw[i][0] + s.aw[i][2];
    return tr;
}

// trace of Scheduler.cov_matrix (kf_workers.py:112-147) for one candidate sensor.  The first
// row of both H_gps and H_imu is e_0 (pos_x), with R[0,0] = 3 (GPS) or 50 (IMU); a full update
// uses every row.  The state vector is not needed, so a zero one is carried through.
template <typename T, bool CUSTOM>
__device__ __forceinline__ Ref15<T, CUSTOM> posterior(const Ref15<T, CUSTOM>& s0, int type, bool full) {
    Ref15<T, CUSTOM> c = s0;
#pragma unroll
    for (int i = 0; i < 15; ++i) c.x[i] = T(0);
    if (!full) {
        T xb[3] = {T(0), T(0), T(0)};
        const T z[1] = {T(0)};
        T q[3], Rp[6], rg;
        pva_noise<CUSTOM, M15>(s0.kc, 0, q, Rp, rg);
        const T R[1] = {type == kGps ? rg : Rp[0]};
        sel_update<3, 1, true, T, kRefNewton, true, kRefJoseph<T>, kRefGainR>(xb, c.pva[0], z, R);
    } else if (type == kGps) {
        const T z[3] = {T(0), T(0), T(0)};
        c.update_gps(z);
    } else {
        T imu[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) imu[i] = T(0);
        c.update_imu(imu, T(0));
    }
    return c;
}

template <typename T, bool CUSTOM>
__device__ __forceinline__ T posterior_trace(const Ref15<T, CUSTOM>& s0, int type, bool full) {
    return cov_trace(posterior(s0, type, full));
}

// One scalar measurement of state k of a chain block with variance r: P -= P e_k e_k^T P / (P_kk + r)
// (Scheduler.cov_matrix's Sigma - K H Sigma for a one-row H, kf_workers.py:121-147)
template <int NB, typename T>
__device__ __forceinline__ void chain_scalar_update(T (&Pb)[NB * (NB + 1) / 2], int k, T r) {
    T g[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) g[i] = Pb[tri<NB>(i, k)];
    const T inv = T(1) / (g[k] + r);
#pragma unroll
    for (int i = 0; i < NB; ++i)
#pragma unroll
        for (int j = i; j < NB; ++j) Pb[tri<NB>(i, j)] = fmaT(-g[i] * inv, g[j], Pb[tri<NB>(i, j)]);
}

// Scheduler.cov_matrix(S, Sigma, R, H) for any set S of measurement rows (kf_workers.py:121-138:
// H_hat = H[S], R_hat = R[S, S]).  H's rows select states and R is diagonal, so the rows are
// independent measurements and, P being block-diagonal over the chains, each chain takes its own
// rows: sequential scalar updates in row order give the joint update's value.  mask bit i = row
// i + 1 of the sensor's H (GPS: pos_x, pos_y, pos_z; IMU: state i).
template <typename T, bool CUSTOM>
__device__ __forceinline__ Ref15<T, CUSTOM> posterior_rows(const Ref15<T, CUSTOM>& s0, int type, uint32_t mask) {
    Ref15<T, CUSTOM> c = s0;
#pragma unroll
    for (int ch = 0; ch < M15::NP; ++ch) {
        T q[3], Rp[6], rg;
        pva_noise<CUSTOM, M15>(s0.kc, ch, q, Rp, rg);
        if (type == kGps) {
            if (mask >> ch & 1u) chain_scalar_update<3>(c.pva[ch], 0, rg);
        } else {
            const T r[3] = {Rp[0], Rp[3], Rp[5]};
#pragma unroll
            for (int k = 0; k < 3; ++k)
                if (mask >> M15::pva(ch, k) & 1u) chain_scalar_update<3>(c.pva[ch], k, r[k]);
        }
    }
    if (type != kGps) {
#pragma unroll
        for (int ch = 0; ch < M15::NA; ++ch) {
            T q[2], Ra[3];
            aw_noise<CUSTOM, M15>(s0.kc, ch, q, Ra);
            const T r[2] = {Ra[0], Ra[2]};
#pragma unroll
            for (int k = 0; k < 2; ++k)
                if (mask >> M15::aw(ch, k) & 1u) chain_scalar_update<2>(c.aw[ch], k, r[k]);
        }
    }
    return c;
}

// The greedy scheduler's gain (S = [1]): only the x-axis (pos, vel, acc) block changes, so the
// trace is the current one with that block's diagonal replaced — no copy of the whole state.
template <typename T, bool CUSTOM>
__device__ __forceinline__ T first_row_gain(const Ref15<T, CUSTOM>& s, int type) {
    T p[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = s.pva[0][k];
    T xb[3] = {T(0), T(0), T(0)};
    const T z[1] = {T(0)};
    T q[3], Rp[6], rg;
    pva_noise<CUSTOM, M15>(s.kc, 0, q, Rp, rg);
    const T R[1] = {type == kGps ? rg : Rp[0]};
    sel_update<3, 1, true, T, kRefNewton, true, kRefJoseph<T>, kRefGainR>(xb, p, z, R);
    T tr = p[0] + p[3] + p[5];
#pragma unroll
    for (int i = 1; i < 3; ++i) tr += s.pva[i][0] + s.pva[i][3] + s.pva[i][5];
#pragma unroll
    for (int i = 0; i < 3; ++i) tr += s.aw[i][0] + s.aw[i][2];
    return tr;
}

template <typename T, bool CUSTOM>
__global__ __launch_bounds__(kBlock) void ref15_score_kernel(const Ref15ScoreArgs a) {
    const int64_t f = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (f >= a.B) return;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(a.B) * uint32_t(sizeof(T));
    const uint32_t rb_post = a.post ? rb : 0u;
    Ref15<T, CUSTOM> s;
    s.kc = a.kc;
    s.load(a.x, a.P, rb, off);
    for (int c = 0; c < a.n_types; ++c) {
        const Ref15<T, CUSTOM> p = a.rows ? posterior_rows(s, int(a.types[c]), a.masks[c])
                                          : posterior(s, int(a.types[c]), a.full != 0);
        stb(a.gain, c, rb, off, cov_trace(p));
        p.store_cov(a.post, int64_t(c) * 27, rb_post, off);
    }
}

// Scheduler.random_schedule (kf_workers.py:188-193) is np.random.choice(len(queue)) on NumPy's
// global legacy RandomState: randint(0, n) by masked rejection on 32-bit MT19937 outputs (n = 1
// takes no output; otherwise mask = the smallest 2^k - 1 >= n - 1, outputs & mask until one is
// <= n - 1).  The caller hands each filter its column of the generator's raw outputs
// (words[n_words][B]); wp counts the ones taken.  Returns the draw, or -1 when the column ran out.
__device__ __forceinline__ int legacy_choice(const uint32_t* words, int n_words, int64_t B, int64_t f, int& wp, int n) {
    const uint32_t rng = uint32_t(n - 1);
    if (rng == 0) return 0;
    uint32_t mask = rng;
    mask |= mask >> 1;
    mask |= mask >> 2;
    mask |= mask >> 4;
    mask |= mask >> 8;
    mask |= mask >> 16;
    while (wp < n_words) {
        const uint32_t v = words[int64_t(wp++) * B + f] & mask;
        if (v <= rng) return int(v);
    }
    return -1;
}

// the r-th queued event of a queue that began at event `first`: every event from there on that is
// not padding was queued (a trigger ends the queue; an empty queue's trigger is its only event)
__device__ __forceinline__ int queued_event(const uint8_t* etype, int64_t B, int64_t f, int first, int r) {
    for (int ev = first;; ++ev)
        if (etype[int64_t(ev) * B + f] != 255 && r-- == 0) return ev;
}

// The greedy pick needs no scan of the queue: a candidate's gain depends only on its sensor
// type and the current covariance, so the first candidate with the largest gain is the first
// queued GPS fix or the first queued other event (ties: whichever came first; a NaN gain is
// never picked, and with none pickable the queue's first event is, as the reference's loop
// leaves best_i at its start).  Each lane tracks those two candidates (index, type, time) as
// events are queued, and reads the payload of the picked one only.
template <typename T, bool CUSTOM>
struct SchedLane {
    Ref15<T, CUSTOM> s;
    int32_t st;
    double prev, period;
    int q_len = 0, nsel = 0;
    // per class (0: GPS fix, 1: any other event) the first queued event's index (-1: none),
    // type and time; named scalars, not arrays (an array indexed by a runtime class went to
    // scratch memory)
    int qi0 = -1, qi1 = -1, qt0 = 0, qt1 = 0;
    double qtime0 = 0.0, qtime1 = 0.0;
    int q_first = 0, wp = 0;  // random selection: the queue's first event, generator outputs taken (-1: ran out)

    // event i (type ty at time ti) of filter f (kf_workers.py:870-957)
    __device__ __forceinline__ void event(const Ref15SchedArgs& a, int64_t f, int i, int ty, double ti) {
        if (ty == 255 || wp < 0) return;  // padding of a ragged stream; a random run out of draws
        const int64_t B = a.B;
        const bool gps = ty == kGps;
        const bool window = ti - prev < period;  // still inside the window: queue it
        if (window || q_len == 0) {  // a trigger with an empty queue is its own candidate
            if (q_len == 0) q_first = i;
            if (gps && qi0 < 0) {
                qi0 = i;
                qt0 = ty;
                qtime0 = ti;
            }
            if (!gps && qi1 < 0) {
                qi1 = i;
                qt1 = ty;
                qtime1 = ti;
            }
            ++q_len;
            if (window) return;
        }
        // greedy_schedule (kf_workers.py:195-213); with one class queued its first event is
        // the pick whatever the gain (a NaN gain leaves the queue's first, the same event)
        bool pick0 = qi0 >= 0;
        if (qi0 >= 0 && qi1 >= 0 && !a.words) {
            const T g0 = first_row_gain(s, kGps), g1 = first_row_gain(s, kImu);
            const bool v0 = g0 == g0, v1 = g1 == g1;
            if (v0 && v1) pick0 = g0 > g1 ? true : (g1 > g0 ? false : qi0 < qi1);
            else if (v0 != v1) pick0 = v0;
            else pick0 = qi0 < qi1;  // the queue's first
        }
        int sel = pick0 ? qi0 : qi1;
        double tsel = pick0 ? qtime0 : qtime1;
        int tsel_type = pick0 ? qt0 : qt1;
        if (a.words) {  // random_schedule: any queued event, drawn as the reference draws it
            const int r = legacy_choice(a.words, a.n_words, B, f, wp, q_len);
            if (r < 0) {
                wp = -1;
                return;
            }
            sel = queued_event(a.etype, B, f, q_first, r);
            tsel = a.t[int64_t(sel) * B + f];
            tsel_type = a.etype[int64_t(sel) * B + f];
        }
        q_len = 0;
        qi0 = qi1 = -1;
        T pay[9];
        // the selected event differs per lane: plain 64-bit addressing (a buffer descriptor per
        // lane would be a waterfall loop)
        // [T][9][B] rows, or [T][B][pay_rec] records (kf_run_scheduled_rec)
        const T* ps = static_cast<const T*>(a.payload) +
                      (a.pay_rec ? (int64_t(sel) * B + f) * a.pay_rec : int64_t(sel) * 9 * B + f);
        const int64_t pstep = a.pay_rec ? 1 : B;
#pragma unroll
        for (int k = 0; k < 9; ++k) pay[k] = ps[int64_t(k) * pstep];
        bool ok = true;
        s.template event<false>(tsel_type, T(tsel - prev), pay, false, T(0), ok);
        if (!ok) {
            st = kNotSpd;
            s.fill_nan();
        }
        if (a.traj) {
            T* tro = static_cast<T*>(a.traj) + int64_t(nsel) * 6 * B + f;
#pragma unroll
            for (int k = 0; k < 6; ++k) tro[int64_t(k) * B] = s.x[k];
        }
        if (a.logdet) static_cast<T*>(a.logdet)[int64_t(nsel) * B + f] = s.logdet();
        if (a.sel_time) a.sel_time[int64_t(nsel) * B + f] = tsel;
        ++nsel;
        prev = tsel;
    }
};

// random_schedule's picks alone (kf_sched_random_picks): the windows and the draws need only the
// event times and types (the windows open at the picked events' times, the draws consume the
// filter's generator outputs), so a lane per filter walks its stream with no filter arithmetic
// and writes the picked event indices and times; the caller runs the picked events through the
// event engine (for one filter over a long log: kf_run_events' time-parallel route).  Event
// types and times ride an 8-deep register ring; the generator outputs a 4-deep one.
template <int D>
__device__ __forceinline__ void ring_shift(int (&ty)[D], double (&tt)[D]) {
#pragma unroll
    for (int k = 0; k + 1 < D; ++k) {
        ty[k] = ty[k + 1];
        tt[k] = tt[k + 1];
    }
}
__global__ __launch_bounds__(kBlock) void ref15_random_picks_kernel(const Ref15SchedArgs a, int32_t* pick) {
    const int64_t f = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (f >= a.B) return;
    const int64_t B = a.B;
    constexpr int D = 8;
    int ty[D];
    double tt[D];
#pragma unroll
    for (int k = 0; k < D; ++k) {
        ty[k] = k < a.T ? int(a.etype[int64_t(k) * B + f]) : 255;
        tt[k] = k < a.T ? a.t[int64_t(k) * B + f] : 0.0;
    }
    double prev = a.prev_time[f];
    const double period = 1.0 / (a.freq ? a.freq[f] : a.freq_all);  // kf_workers.py:880
    int q_len = 0, q_first = 0, nsel = 0, wp = 0;
    bool q_gap = false;  // a padding event inside the queue: the r-th queued event needs a scan
    for (int i = 0; i < a.T; ++i) {
        const int ty0 = ty[0];
        const double t0 = tt[0];
        ring_shift(ty, tt);
        const int nx = i + D;
        ty[D - 1] = nx < a.T ? int(a.etype[int64_t(nx) * B + f]) : 255;
        tt[D - 1] = nx < a.T ? a.t[int64_t(nx) * B + f] : 0.0;
        if (ty0 == 255) {  // padding: never queued (a queue it falls inside is no longer contiguous)
            q_gap = q_gap || q_len > 0;
            continue;
        }
        const bool window = t0 - prev < period;
        if (window || q_len == 0) {
            if (q_len == 0) {
                q_first = i;
                q_gap = false;
            }
            ++q_len;
            if (window) continue;
        }
        const int r = legacy_choice(a.words, a.n_words, B, f, wp, q_len);
        if (r < 0) {
            wp = -1;
            break;
        }
        const int sel = q_gap ? queued_event(a.etype, B, f, q_first, r) : q_first + r;
        const double ts = sel == i ? t0 : a.t[int64_t(sel) * B + f];
        pick[int64_t(nsel) * B + f] = sel;
        a.sel_time[int64_t(nsel) * B + f] = ts;
        ++nsel;
        prev = ts;
        q_len = 0;
    }
    a.n_sel[f] = nsel;
    a.words_used[f] = wp;
}

#ifndef KF_SCHED_WAVES
#define KF_SCHED_WAVES 2
#endif
// Any B: the next event's type and time are loaded one event ahead in registers.
template <typename T, bool CUSTOM>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(KF_SCHED_WAVES))) void ref15_sched_kernel(
    const Ref15SchedArgs a) {
    const int64_t f = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (f >= a.B) return;
    if (a.only && !a.only[f]) return;  // the two-pass run's fallback: flagged filters only
    const int64_t B = a.B;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(B) * uint32_t(sizeof(T));
    SchedLane<T, CUSTOM> L;
    L.s.kc = a.kc;
    L.s.load(a.x, a.P, rb, off);
    L.st = a.status[f];
    L.prev = a.prev_time[f];
    L.period = 1.0 / (a.freq ? a.freq[f] : a.freq_all);  // kf_workers.py:880
    int tyn = a.T > 0 ? a.etype[f] : 255;
    double tn = a.T > 0 ? a.t[f] : 0.0;
    for (int i = 0; i < a.T; ++i) {
        const int ty = tyn;
        const double ti = tn;
        if (i + 1 < a.T) {
            tyn = a.etype[int64_t(i + 1) * B + f];
            tn = a.t[int64_t(i + 1) * B + f];
        }
        L.event(a, f, i, ty, ti);
    }
    if (a.n_sel) a.n_sel[f] = L.nsel;
    if (a.words_used) a.words_used[f] = L.wp;
    L.s.store(a.x, a.P, rb, off);
    a.status[f] = L.st;
}

// B % 64 == 0: the event types and times travel HBM -> LDS by buffer_load ... lds, kSchedChunk
// events at a time into one of two per-wave images while the previous chunk is consumed (the
// queueing iterations are a few instructions each, so a register prefetch one event ahead
// waited a memory latency per event, and a deeper one did not fit the registers).
//   image: t rows [kSchedChunk][64] f64, then etype rows [kSchedChunk][64] u8
#ifndef KF_SCHED_CHUNK
#define KF_SCHED_CHUNK 16
#endif
constexpr int kSchedChunk = KF_SCHED_CHUNK;
constexpr int kSchedImg = kSchedChunk * 512 + kSchedChunk * 64;
template <typename T, bool CUSTOM>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(KF_SCHED_WAVES))) void ref15_sched_lds_kernel(
    const Ref15SchedArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * 2 * kSchedImg];
    const int lane = int(threadIdx.x & 63);
    const int wave = wave_uniform(int(threadIdx.x >> 6));
    const int64_t f0 = int64_t(blockIdx.x) * kBlock + int64_t(wave) * 64;
    if (f0 >= a.B) return;  // whole waves (B % 64 == 0)
    const int64_t f = f0 + lane;
    const int64_t B = a.B;
    unsigned char* const img0 = lds + wave * 2 * kSchedImg;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(B) * uint32_t(sizeof(T));
    SchedLane<T, CUSTOM> L;
    L.s.kc = a.kc;
    L.s.load(a.x, a.P, rb, off);
    L.st = a.status[f];
    L.prev = a.prev_time[f];
    L.period = 1.0 / (a.freq ? a.freq[f] : a.freq_all);
    waitcnt<vmcnt_imm(0)>();
    // t: one 16-B-per-lane DMA moves two rows (lanes 0-31 row r, 32-63 row r + 1); etype: one
    // moves 16 rows of 64 bytes (4 lanes per row)
    const uint32_t voff_t = uint32_t(lane >> 5) * uint32_t(B) * 8u + uint32_t(lane & 31) * 16u;
    const uint32_t voff_e = uint32_t(lane >> 2) * uint32_t(B) + uint32_t(lane & 3) * 16u;
    auto issue = [&](int c, unsigned char* img) {
        const int r0 = c * kSchedChunk;
        const int nr = a.T - r0 < kSchedChunk ? a.T - r0 : kSchedChunk;  // rows of this chunk (>= 1)
#pragma unroll
        for (int k = 0; k < kSchedChunk / 2; ++k) {
            if (2 * k >= nr) break;  // wave-uniform
            const char* tb = reinterpret_cast<const char*>(a.t) + (int64_t(r0 + 2 * k) * B + f0) * 8;
            const uint32_t span = 2 * k + 1 < nr ? uint32_t(B) * 8u + 512u : 512u;
            lds_dma16(bytes_rsrc(tb, span), img + k * 1024, voff_t, 0);
        }
        const char* eb = reinterpret_cast<const char*>(a.etype) + int64_t(r0) * B + f0;
        lds_dma16(bytes_rsrc(eb, uint32_t(nr - 1) * uint32_t(B) + 64u), img + kSchedChunk * 512, voff_e, 0);
    };
    const int nch = (a.T + kSchedChunk - 1) / kSchedChunk;
    if (nch > 0) issue(0, img0);
    for (int c = 0; c < nch; ++c) {
        // this chunk's image has landed, the other image's reads are done (vmcnt also counts
        // the stores of the chunk before: once per chunk)
        waitcnt<0>();
        unsigned char* const img = img0 + (c & 1) * kSchedImg;
        if (c + 1 < nch) issue(c + 1, img0 + ((c + 1) & 1) * kSchedImg);
        const double* ti_img = reinterpret_cast<const double*>(img) + lane;
        const unsigned char* ty_img = img + kSchedChunk * 512 + lane;
        const int r0 = c * kSchedChunk;
        const int nr = a.T - r0 < kSchedChunk ? a.T - r0 : kSchedChunk;
#pragma unroll 1
        for (int d = 0; d < nr; ++d) L.event(a, f, r0 + d, int(ty_img[d * 64]), ti_img[d * 64]);
    }
    if (a.n_sel) a.n_sel[f] = L.nsel;
    if (a.words_used) a.words_used[f] = L.wp;
    L.s.store(a.x, a.P, rb, off);
    a.status[f] = L.st;
}

// ------------------------------------------------------------------------------------
// Two-pass scheduled filter.  The greedy pick (kf_workers.py:195-213) compares two posterior
// traces tr(P) - |P e_0|^2 / (P_00 + R) whose only difference is R: R_gps[0] for a fix, R_imu[0]
// for any other event.  Wherever the covariance is finite the pick is therefore decided by the
// constants alone — the larger R gives the larger trace — so the windows, the queue and the
// picks need no covariance at all.  Pass 1 (ref15_pick_kernel) runs them from the event times
// and types only (registers for a handful of scalars, 8 waves per SIMD) and writes each pick as
// code << 24 | event index (code: event type, both-classes-queued bit, fix-first bit) with its
// time.  Pass 2 (ref15_apply_kernel) runs the picked events as the fused kernel's apply does,
// the picked payload rows gathered HBM -> LDS by DMA one pick ahead, and at every pick made with
// both classes queued it evaluates the two gains on the covariance, as the fused kernel does: if
// the greedy rule disagrees (a NaN covariance, a rounding tie) the filter is flagged and left
// untouched, and the fused kernel reruns exactly those filters.  Outputs are the fused kernel's.
// ------------------------------------------------------------------------------------
constexpr int kPickBoth = 0x10, kPickGpsFirst = 0x20;

// payload element i of this lane in the apply pass's image, read from LDS where the update uses
// it.  Rows ([T][9][B]): [9][64] slots of kSlot bytes per lane.  Records ([T][B][rec],
// REC): the first 9 values of the lane's record as 16-B chunks, [chunk][64][16 B].
template <typename T, bool REC = false>
struct LdsGathered {
    const unsigned char* img;  // image base + this lane's slot (+ its value's offset in the slot)
    static constexpr int kSlot = REC || sizeof(T) == 8 ? 16 : 4;
    static constexpr int kChunks = (9 * int(sizeof(T)) + 15) / 16;  // REC: 16-B chunks per record
    __device__ __forceinline__ T operator[](int i) const {
        constexpr int W = int(sizeof(T));
        if constexpr (REC) return *reinterpret_cast<const T*>(img + ((i * W) >> 4) * 1024 + ((i * W) & 15));
        else return *reinterpret_cast<const T*>(img + i * 64 * kSlot);
    }
};

#ifndef KF_PICK_CHUNK
#define KF_PICK_CHUNK 8
#endif
#ifndef KF_APPLY_IMAGES
#define KF_APPLY_IMAGES 1  // payload images per wave of the two-pass apply (2: two-wave groups)
#endif
#ifndef KF_REC_IMAGES
#define KF_REC_IMAGES 1  // payload images per wave of the apply pass over payload records (2: A/B)
#endif
#ifndef KF_APPLY_PROBE
#define KF_APPLY_PROBE 0  // 1 / 2 / 3: apply-pass timing probes for in-process A/B builds (tools/ab_inproc.py)
#endif
// events per LDS image of the pick pass: its lanes hold a few scalars, so the LDS, not the
// registers, sets its waves per SIMD (8 events: 4 workgroups of 4 waves per CU)
constexpr int kPickChunk = KF_PICK_CHUNK;
constexpr int kPickImg = kPickChunk * 512 + kPickChunk * 64;
// The pick pass of one wave (filters f0 .. f0 + 63) with its two staging images at img0
// (2 * kPickImg bytes); returns this lane's pick count.  Every store is issued on return.
// RND: random_schedule's pick (a.words) instead of the greedy rule's; picks carry no
// both-classes bit, so the apply pass checks nothing and flags no filter.
template <bool RND = false>
__device__ __forceinline__ int pick_phase(const Ref15SchedArgs& a, int lane, int64_t f0, unsigned char* img0) {
    constexpr int kSchedChunk = kPickChunk, kSchedImg = kPickImg;  // the fused kernel's staging, resized
    static_assert(kSchedChunk % 2 == 0 && kSchedChunk <= 16, "t rows move in pairs; etype rows 4 lanes each");
    const int64_t f = f0 + lane;
    const int64_t B = a.B;
    double prev = a.prev_time[f];
    const double period = 1.0 / (a.freq ? a.freq[f] : a.freq_all);  // kf_workers.py:880
    int q_len = 0, nsel = 0, qi0 = -1, qi1 = -1, qt0 = 0, qt1 = 0;
    double qtime0 = 0.0, qtime1 = 0.0;
    int q_first = 0, wp = 0;  // RND: the queue's first event, generator outputs taken (-1: ran out)
    waitcnt<vmcnt_imm(0)>();
    const uint32_t voff_t = uint32_t(lane >> 5) * uint32_t(B) * 8u + uint32_t(lane & 31) * 16u;
    const uint32_t voff_e = uint32_t(lane >> 2) * uint32_t(B) + uint32_t(lane & 3) * 16u;
    auto issue = [&](int c, unsigned char* img) {
        const int r0 = c * kSchedChunk;
        const int nr = a.T - r0 < kSchedChunk ? a.T - r0 : kSchedChunk;
#pragma unroll
        for (int k = 0; k < kSchedChunk / 2; ++k) {
            if (2 * k >= nr) break;  // wave-uniform
            const char* tb = reinterpret_cast<const char*>(a.t) + (int64_t(r0 + 2 * k) * B + f0) * 8;
            const uint32_t span = 2 * k + 1 < nr ? uint32_t(B) * 8u + 512u : 512u;
            lds_dma16(bytes_rsrc(tb, span), img + k * 1024, voff_t, 0);
        }
        // 4 lanes per etype row: the lanes past this chunk's rows would write zeros (their rows
        // are out of the descriptor's range) beyond the image
        const char* eb = reinterpret_cast<const char*>(a.etype) + int64_t(r0) * B + f0;
        if (lane < 4 * kSchedChunk)
            lds_dma16(bytes_rsrc(eb, uint32_t(nr - 1) * uint32_t(B) + 64u), img + kSchedChunk * 512, voff_e, 0);
    };
    const int nch = (a.T + kSchedChunk - 1) / kSchedChunk;
    if (nch > 0) issue(0, img0);
    for (int c = 0; c < nch; ++c) {
        waitcnt<0>();
        unsigned char* const img = img0 + (c & 1) * kSchedImg;
        if (c + 1 < nch) issue(c + 1, img0 + ((c + 1) & 1) * kSchedImg);
        const double* ti_img = reinterpret_cast<const double*>(img) + lane;
        const unsigned char* ty_img = img + kSchedChunk * 512 + lane;
        const int r0 = c * kSchedChunk;
        const int nr = a.T - r0 < kSchedChunk ? a.T - r0 : kSchedChunk;
#pragma unroll 1
        for (int d = 0; d < nr; ++d) {
            const int ty = int(ty_img[d * 64]);
            const double ti = ti_img[d * 64];
            const int i = r0 + d;
            if (ty == 255 || (RND && wp < 0)) continue;  // padding of a ragged stream; out of draws
            const bool gps = ty == kGps;
            const bool window = ti - prev < period;  // SchedLane::event, kf_workers.py:870-957
            if (window || q_len == 0) {
                if (RND && q_len == 0) q_first = i;
                if (gps && qi0 < 0) {
                    qi0 = i;
                    qt0 = ty;
                    qtime0 = ti;
                }
                if (!gps && qi1 < 0) {
                    qi1 = i;
                    qt1 = ty;
                    qtime1 = ti;
                }
                ++q_len;
                if (window) continue;
            }
            const bool both = qi0 >= 0 && qi1 >= 0;
            const bool gps_first = qi0 >= 0 && (qi1 < 0 || qi0 < qi1);
            const bool pick0 = both ? (a.gps_wins > 0 ? true : a.gps_wins == 0 ? false : gps_first) : qi0 >= 0;
            int sel = pick0 ? qi0 : qi1;
            double tsel = pick0 ? qtime0 : qtime1;
            int code = (pick0 ? qt0 : qt1) | (both ? kPickBoth : 0) | (gps_first ? kPickGpsFirst : 0);
            if constexpr (RND) {
                const int r = legacy_choice(a.words, a.n_words, B, f, wp, q_len);
                if (r < 0) {
                    wp = -1;
                    continue;
                }
                sel = queued_event(a.etype, B, f, q_first, r);
                tsel = a.t[int64_t(sel) * B + f];
                code = a.etype[int64_t(sel) * B + f];
            }
            a.picks[int64_t(nsel) * B + f] = (uint32_t(code) << 24) | uint32_t(sel);
            if (a.sel_time && !a.rec_time) a.sel_time[int64_t(nsel) * B + f] = tsel;  // rec_time: the apply pass writes it
            ++nsel;
            prev = tsel;
            q_len = 0;
            qi0 = qi1 = -1;
        }
    }
    if (a.n_sel) a.n_sel[f] = nsel;
    if (RND && a.words_used) a.words_used[f] = wp;
    a.flags[f] = 0;
    return nsel;
}

template <int WAVES, bool RND = false>
__global__ __launch_bounds__(WAVES * 64) void ref15_pick_kernel(const Ref15SchedArgs a) {
    __shared__ __attribute__((aligned(16))) unsigned char lds[WAVES * 2 * kPickImg];
    const int lane = int(threadIdx.x & 63);
    const int wave = WAVES == 1 ? 0 : wave_uniform(int(threadIdx.x >> 6));
    const int64_t f0 = int64_t(blockIdx.x) * (WAVES * 64) + int64_t(wave) * 64;
    if (f0 >= a.B) return;  // whole waves (B % 64 == 0)
    const int nsel = pick_phase<RND>(a, lane, f0, lds + wave * 2 * kPickImg);
    if (a.wave_key) {  // the wave's longest pick list, for the apply pass's heaviest-first order
        int S = nsel;
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) {
            const int o = __shfl_xor(S, sh, 64);
            S = o > S ? o : S;
        }
        if (lane == 0) {
            a.wave_key[f0 >> 6] = uint32_t(S);
            a.wave_id[f0 >> 6] = uint32_t(f0 >> 6);
        }
    }
}

// The one-launch run's wave order: its picks do not exist before the launch, so each wave is
// keyed by its highest processing frequency, which sets its pick count (bit patterns of
// positive floats sort as their values).
__global__ __launch_bounds__(kBlock) void ref15_rate_key_kernel(const Ref15SchedArgs a) {
    const int lane = int(threadIdx.x & 63);
    const int64_t f0 = int64_t(blockIdx.x) * kBlock + int64_t(threadIdx.x >> 6) * 64;
    if (f0 >= a.B) return;  // whole waves (B % 64 == 0)
    float fr = float(a.freq[f0 + lane]);
    fr = fr > 0.0f ? fr : 0.0f;  // NaN and non-positive rates sort last
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const float o = __shfl_xor(fr, sh, 64);
        fr = o > fr ? o : fr;
    }
    if (lane == 0) {
        a.wave_key[f0 >> 6] = __float_as_uint(fr);
        a.wave_id[f0 >> 6] = uint32_t(f0 >> 6);
    }
}

// PICK: the wave runs its pick pass first (one launch for both passes: a wave's streaming pick
// phase overlaps the other waves' compute-bound apply phases)
// REC: the payload is [T][B][pay_rec] records (kf_run_scheduled_rec): a lane's 9 values are one
// contiguous 72-B (f64) span, gathered as 16-B chunks, instead of 9 rows B elements apart
// RT: f64 records carry the event's time at rec[9] (KF_OPT_SCHED_REC_TIME): each pick's time
// comes with its gathered record (the 16-B chunk holding payload[8] already spans it) instead of
// a sel_time row read, and this pass writes sel_time; two payload images, so pick q + 1's record
// (and time) is in flight through event q
template <typename T, bool CUSTOM, int WAVES, bool PICK, bool REC = false, bool RT = false>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu(3))) void ref15_apply_kernel(
    const Ref15SchedArgs a) {
    static_assert(!RT || (REC && sizeof(T) == 8 && !PICK), "record time: f64 records, two launches");
    constexpr int W = int(sizeof(T));
    // The picked payload is gathered per lane: the picks of a wave's lanes lie on different rows,
    // so with the [T][9][B] rows every gather instruction touches up to 64 cache lines and the
    // address unit, not HBM, bounds the pass.  f64 moves 16 B per lane (the aligned pair holding
    // the lane's value: one instruction per value instead of two dword ones), f32 4 B.  With
    // records (REC) a pick is 5 (f64) / 3 (f32) 16-B chunks of one span, and the pass moves its
    // bytes at the HBM's rate.  One payload image per wave:
    // the next pick's gather is issued once this event's update has read the image, and waited
    // for after the next predict.
    // NIMG = 2: two payload images, pick q + 1's gather issued before event q's predict (a whole
    // event of cover instead of one predict), at the LDS cost of fewer waves per CU
    // (records: 5-KB images, so two fit 12 waves per CU, KF_REC_IMAGES=2: measured no faster)
    constexpr int NIMG = RT ? 2 : PICK ? 1 : REC ? KF_REC_IMAGES : KF_APPLY_IMAGES;
    static_assert(NIMG == 1 || NIMG == 2, "payload images");
    using Gathered = LdsGathered<T, REC>;
    constexpr int GB = Gathered::kSlot;
    constexpr int PAY = REC ? Gathered::kChunks * 1024 : 9 * 64 * GB;  // payload image
    constexpr int NG = REC ? Gathered::kChunks : 9;                     // gather instructions per pick
    constexpr int TM = NIMG * PAY;         // pick times, two rows (q & 1)
    constexpr int PK = TM + 2 * 512;       // picks, three rows (q % 3), 64 u32 each
    constexpr int APPLY_LDS = PK + 3 * 256;
    constexpr int WAVE_LDS = PICK && 2 * kPickImg > APPLY_LDS ? 2 * kPickImg : APPLY_LDS;  // the pick phase's images alias
    constexpr int NST = RT ? 8 : 7;        // traj (6 rows), logdet (RT: sel_time); absent ones dropped by offset
    __shared__ __attribute__((aligned(16))) unsigned char lds[WAVES * WAVE_LDS];
    const int lane = int(threadIdx.x & 63);
    const int wave = WAVES == 1 ? 0 : wave_uniform(int(threadIdx.x >> 6));
    const int64_t slot = int64_t(blockIdx.x) * WAVES + wave;  // the wave's place in the launch
    if (slot * 64 >= a.B) return;  // whole waves (B % 64 == 0)
    // heaviest waves first where the pick pass sorted them (their list lengths differ by rate,
    // and the longest started last set the launch's tail)
    const int64_t f0 = (a.order ? int64_t(wave_uniform(int(a.order[slot]))) : slot) * 64;
    const int64_t f = f0 + lane;
    const int64_t B = a.B;
    unsigned char* const base = lds + wave * WAVE_LDS;
    const uint32_t off = uint32_t(f) * uint32_t(W);
    const uint32_t rb = uint32_t(B) * uint32_t(W);
    int nsel;
    if constexpr (PICK) {
        nsel = pick_phase(a, lane, f0, base);
        waitcnt<vmcnt_imm(0)>();  // its picks are read back below (this wave's own rows)
    } else {
        nsel = a.n_sel[f];
    }
    Ref15<T, CUSTOM> s;
    s.kc = a.kc;
    s.load(a.x, a.P, rb, off);
    int32_t st = a.status[f];
    double prev = a.prev_time[f];
    int S = nsel;  // the wave's longest pick list
#pragma unroll
    for (int sh = 32; sh >= 1; sh >>= 1) {
        const int o = __shfl_xor(S, sh, 64);
        S = o > S ? o : S;
    }
    S = wave_uniform(S);
    waitcnt<vmcnt_imm(0)>();
    // pick r's payload (NG VMEM): a lane past its list reads row 0.  Device pass only: the 16-B
    // form of the builtin is a gfx950 one, and the host pass would drop the kernel's stub.
    auto gather = [&](int r, uint32_t pick) {
#if defined(__HIP_DEVICE_COMPILE__)
        const int64_t col = W == 8 ? (f & ~int64_t(1)) : f;  // f64: the 16-B-aligned pair
        const uint32_t ev = pick & 0xFFFFFFu;
#if KF_APPLY_PROBE == 1  // timing probe (wrong results): every lane gathers lane 0's row
        const int64_t row = __shfl((r < nsel && ev < uint32_t(a.T)) ? int(ev) : 0, 0, 64);
#else
        const int64_t row = (r < nsel && ev < uint32_t(a.T)) ? int64_t(ev) : 0;
#endif
        if constexpr (REC) {  // the record's first kChunks 16-B chunks (within pay_rec * W bytes)
            const char* src = reinterpret_cast<const char*>(a.payload) + (row * B + f) * int64_t(a.pay_rec) * W;
#pragma unroll
            for (int c = 0; c < Gathered::kChunks; ++c)
                __builtin_amdgcn_global_load_lds(src + c * 16,
                                                 (__attribute__((address_space(3))) void*)(base + (r & (NIMG - 1)) * PAY + c * 1024),
                                                 16, 0, 0);
        } else {
            const char* src = reinterpret_cast<const char*>(a.payload) + (row * 9 * B + col) * W;
#pragma unroll
            for (int i = 0; i < 9; ++i)
#if KF_APPLY_PROBE == 2  // timing probe (wrong results): no payload gather
                if (r < 0)
#endif
                    __builtin_amdgcn_global_load_lds(src + int64_t(i) * B * W,
                                                     (__attribute__((address_space(3))) void*)(base + (r & (NIMG - 1)) * PAY + i * 64 * GB),
                                                     Gathered::kSlot, 0, 0);
        }
#else
        (void)r;
        (void)pick;
#endif
    };
    // pick r's time / row r of the picks (1 VMEM each, issued by every wave: past the list a
    // zero-length descriptor, so the waits below can be counted)
    auto issue_time = [&](int r) {
        const char* tb = reinterpret_cast<const char*>(a.sel_time) + (int64_t(r) * B + f0) * 8;
        if (lane < 32) lds_dma16(bytes_rsrc(tb, r < S ? 512u : 0u), base + TM + (r & 1) * 512, uint32_t(lane) * 16u, 0);
    };
    auto issue_picks = [&](int r) {
        const char* pb = reinterpret_cast<const char*>(a.picks) + (int64_t(r) * B + f0) * 4;
        if (lane < 16) lds_dma16(bytes_rsrc(pb, r < S ? 256u : 0u), base + PK + (r % 3) * 256, uint32_t(lane) * 16u, 0);
    };
    auto pick_row = [&](int r) { return reinterpret_cast<const uint32_t*>(base + PK + (r % 3) * 256)[lane]; };
    const unsigned char* const pay0 = base + lane * GB + (!REC && W == 8 ? (lane & 1) * 8 : 0);  // read where used
    if (S > 0) {
        issue_picks(0);
        issue_picks(1);
        if constexpr (!RT) issue_time(0);
        waitcnt<vmcnt_imm(0)>();
        gather(0, pick_row(0));
    }
    bool bad = false;
    for (int q = 0; q < S; ++q) {
        const Gathered pay{pay0 + (q & (NIMG - 1)) * PAY};
        if constexpr (NIMG == 1) {
            // time q and pick row q: older than pick row q + 1, gather q (NG) and event q - 1's stores
            if (q > 0) waitcnt<vmcnt_imm(1 + NG + NST)>();
        } else {
            // time q, pick row q + 1 and gather q: older than event q - 1's stores
            if (q > 0) waitcnt<vmcnt_imm(NST)>();
            // the other image was last read by event q - 1's update
            __builtin_amdgcn_s_waitcnt(lgkmcnt0_imm);
            asm volatile("" ::: "memory");
            if (q + 1 < S) gather(q + 1, pick_row(q + 1));
            // RT: the time is in record q (gather 0 is older than gather 1, when there is one)
            if (RT && q == 0) {
                if (S > 1) waitcnt<vmcnt_imm(NG)>();
                else waitcnt<vmcnt_imm(0)>();
            }
        }
        double tq;
        if constexpr (RT) tq = pay[9];
        else tq = reinterpret_cast<const double*>(base + TM + (q & 1) * 512)[lane];
        const uint32_t pick_c = pick_row(q);
        if constexpr (!RT) issue_time(q + 1);
        issue_picks(q + 2);  // into the slot row q - 1 held
        const bool live = q < nsel;
        const int code = int(pick_c >> 24);
#if KF_APPLY_PROBE == 3  // timing probe (wrong results): lane 0's event type for the wave
        const int type = __shfl(code & 7, 0, 64);
#else
        const int type = code & 7;
#endif
        if (live && !bad && (code & kPickBoth)) {
            // the greedy rule on this covariance (SchedLane::event): the pick pass's choice must
            // be the first candidate with the largest gain
            const T g0 = first_row_gain(s, kGps), g1 = first_row_gain(s, kImu);
            const bool v0 = g0 == g0, v1 = g1 == g1;
            const bool gps_first = (code & kPickGpsFirst) != 0;
            bool pick0;
            if (v0 && v1) pick0 = g0 > g1 ? true : (g1 > g0 ? false : gps_first);
            else if (v0 != v1) pick0 = v0;
            else pick0 = gps_first;
#if KF_APPLY_PROBE == 3
            bad = false && pick0;
#else
            bad = pick0 != (type == kGps);
#endif
        }
        const bool run = live && !bad;
        const T dt = T(tq - prev);
        if (run) s.predict(dt);  // Chains::event, split around the payload wait
        if constexpr (NIMG == 1) {
            // gather q: older than event q - 1's stores, time q + 1 and pick row q + 2
            if (q > 0) waitcnt<vmcnt_imm(NST + 2)>();
            else waitcnt<vmcnt_imm(2)>();
        } else if (!RT && q == 0) {
            // gather 0: older than gather 1 (when there is one), time 1 and pick row 2
            if (S > 1) waitcnt<vmcnt_imm(NG + 2)>();
            else waitcnt<vmcnt_imm(2)>();
        }
        if (run && (type == kGps || type == kImu)) {
            bool ok;
            if (type == kGps) {
                const T z[3] = {pay[0], pay[1], pay[2]};  // (easting, northing, altitude)
                ok = s.template update_gps<false>(z);
            } else {
                ok = s.template update_imu<false>(pay, dt);
            }
            if (!ok) {
                st = kNotSpd;
                s.fill_nan();
            }
        }
        if (run) prev = tq;
        // the image's reads are done: gather q + 1 into it (its pick row landed before gather q;
        // reading the payload into registers first, to issue the gather before the update, cost
        // 10 spilled registers and measured 5.98 vs 5.45 ms)
        if constexpr (NIMG == 1) {
            __builtin_amdgcn_s_waitcnt(lgkmcnt0_imm);
            asm volatile("" ::: "memory");
            if (q + 1 < S) gather(q + 1, pick_row(q + 1));
        }
        // a record's descriptor per pick (the records of the whole run exceed 32-bit offsets)
        const uint32_t vo = live ? off : kDropOffset;
        const auto r_tr = span_rsrc(a.traj, int64_t(q) * 6, rb, 6u);
#pragma unroll
        for (int k = 0; k < 6; ++k) stv(r_tr, uint32_t(k) * rb + vo, s.x[k]);
        stv(span_rsrc(a.logdet, q, rb, 1u), vo, s.logdet());
        if constexpr (RT) stv(span_rsrc(a.sel_time, q, rb, 1u), vo, tq);
    }
    a.flags[f] = bad ? 1 : 0;
    if (bad) return;  // the fused kernel reruns this filter from the handle's state
    s.store(a.x, a.P, rb, off);
    a.status[f] = st;
}
}  // namespace

hipError_t launch_ref15_random_picks(const Ref15SchedArgs& a, int32_t* pick, hipStream_t stream) {
    if (a.B <= 0 || a.T < 0 || !a.words || !a.words_used || !a.n_sel || !a.sel_time || !pick) return hipErrorInvalidValue;
    ref15_random_picks_kernel<<<dim3(unsigned((a.B + kBlock - 1) / kBlock)), kBlock, 0, stream>>>(a, pick);
    return hipGetLastError();
}

hipError_t launch_ref15_score(bool f64, const Ref15ScoreArgs& a, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((a.B + kBlock - 1) / kBlock));
    KF_CUSTOM_DISPATCH(a.kc, KF_DTYPE_DISPATCH(f64, ref15_score_kernel<T, CUSTOM><<<grid, kBlock, 0, stream>>>(a)));
    return hipGetLastError();
}

hipError_t launch_ref15_scheduled(bool f64, const Ref15SchedArgs& a, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((a.B + kBlock - 1) / kBlock));
    // the LDS variants' descriptors: whole waves, and a chunk's row spans within 32-bit ranges
    const bool lds = a.B % 64 == 0 && uint64_t(a.B) * 8 * 2 < (uint64_t(1) << 32) &&
                     reinterpret_cast<uintptr_t>(a.t) % 16 == 0 && reinterpret_cast<uintptr_t>(a.etype) % 16 == 0 &&
                     uint64_t(a.B) * kSchedChunk < (uint64_t(1) << 32) && !a.regs;
    // two passes where legal (the host gives them workspace); the pick codes hold 24-bit indices
    // and the apply pass's record of one pick spans a 32-bit byte range
    const bool two = lds && !a.fused && a.picks && a.flags && a.n_sel && a.sel_time && a.T < (1 << 24) &&
                     uint64_t(a.B) * 6u * (f64 ? 8u : 4u) < (uint64_t(1) << 32) &&
                     reinterpret_cast<uintptr_t>(a.sel_time) % 16 == 0 &&
                     ((!f64 && !a.pay_rec) || reinterpret_cast<uintptr_t>(a.payload) % 16 == 0) &&
                     (!a.pay_rec || (int64_t(a.pay_rec) * (f64 ? 8 : 4)) % 16 == 0);
    if (two) {
        // four-wave groups (KF_OPT_SCHED_GROUP): one-wave groups, which free their slot when their
        // wave's pick list ends, measured slower on the bench row (5.51 vs 5.07 ms apply)
        const dim3 g1(static_cast<unsigned>(a.B / 64)), g4(static_cast<unsigned>((a.B + kBlock - 1) / kBlock));
        const bool rnd = a.words != nullptr;
        if (a.one_launch && !rnd) {
            Ref15SchedArgs c = a;  // heaviest first by rate where the filters have their own rates
            c.order = nullptr;
            c.rec_time = false;    // its pick phase's sel_time rows are its apply phase's times
            if (a.order && a.freq) {
                ref15_rate_key_kernel<<<g4, 256, 0, stream>>>(a);
                size_t tb = a.sort_tmp_bytes;
                const hipError_t e = sort_pairs_desc_u32(a.sort_tmp, &tb, a.wave_key, a.wave_key_sorted, a.wave_id,
                                                         a.order, static_cast<int>(a.B / 64), 32, stream);
                if (e != hipSuccess) return e;
                c.order = a.order;
            }
            KF_CUSTOM_DISPATCH(c.kc, KF_BOOL_DISPATCH(c.pay_rec, REC, KF_DTYPE_DISPATCH(f64,
                ref15_apply_kernel<T, CUSTOM, 4, true, REC><<<g4, 256, 0, stream>>>(c))));
        } else {
            if (rnd) ref15_pick_kernel<4, true><<<g4, 256, 0, stream>>>(a);
            else if (a.group_waves == 4) ref15_pick_kernel<4><<<g4, 256, 0, stream>>>(a);
            else ref15_pick_kernel<1><<<g1, 64, 0, stream>>>(a);
            if (a.order) {  // the waves by their longest pick list, descending (stable)
                int bits = 1;
                while ((1 << bits) <= a.T && bits < 31) ++bits;
                size_t tb = a.sort_tmp_bytes;
                const hipError_t e = sort_pairs_desc_u32(a.sort_tmp, &tb, a.wave_key, a.wave_key_sorted, a.wave_id,
                                                         a.order, static_cast<int>(a.B / 64), bits, stream);
                if (e != hipSuccess) return e;
            }
            KF_CUSTOM_DISPATCH(a.kc, KF_DTYPE_DISPATCH(f64, {
                if (a.pay_rec) {  // payload records (kf_run_scheduled_rec): four-wave groups
                    // RT (a.rec_time) is instantiated in fp64 only
                    KF_BOOL_DISPATCH(f64 && a.rec_time, RT, if constexpr (!RT || sizeof(T) == 8)
                        ref15_apply_kernel<T, CUSTOM, 4, false, true, RT><<<g4, 256, 0, stream>>>(a));
                } else
#if KF_APPLY_IMAGES == 2
                if (a.group_waves == 4) {  // two images: 8 waves per CU in LDS
                    const dim3 g2(static_cast<unsigned>((a.B + 127) / 128));
                    ref15_apply_kernel<T, CUSTOM, 2, false><<<g2, 128, 0, stream>>>(a);
                } else
#endif
                if (a.group_waves == 4) {
                    ref15_apply_kernel<T, CUSTOM, 4, false><<<g4, 256, 0, stream>>>(a);
                } else {
                    ref15_apply_kernel<T, CUSTOM, 1, false><<<g1, 64, 0, stream>>>(a);
                }
            }));
        }
        if (rnd) return hipGetLastError();  // random picks are never checked, so none is flagged
        Ref15SchedArgs b = a;  // the flagged filters (usually none: every lane leaves at once)
        b.only = a.flags;
        KF_CUSTOM_DISPATCH(a.kc, KF_DTYPE_DISPATCH(f64, ref15_sched_kernel<T, CUSTOM><<<grid, kBlock, 0, stream>>>(b)));
        return hipGetLastError();
    }
    KF_CUSTOM_DISPATCH(a.kc, KF_DTYPE_DISPATCH(f64, {
        if (lds) ref15_sched_lds_kernel<T, CUSTOM><<<grid, kBlock, 0, stream>>>(a);
        else ref15_sched_kernel<T, CUSTOM><<<grid, kBlock, 0, stream>>>(a);
    }));
    return hipGetLastError();
}

}  // namespace kfmi

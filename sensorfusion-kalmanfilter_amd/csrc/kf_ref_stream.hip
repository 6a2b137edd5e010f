// The time-parallel run of one filter over a long event stream (kf_run_stream), on the reference
// models' layer (kf_ref_model.h): the chunk set-up and perturbation, the scan of the chunks'
// affine state maps, the linear-fractional covariance maps and the chunk starts, the records and
// the final check (launch_stream_phase), and the choice of the sequential fallback's kernel in a
// gated run, the chain kernel or the look-ahead one (launch_stream_choose).
#include "kf_ref_model.h"

namespace kfmi {
namespace {

// ------------------------------------------------------------------------------------
// Time-parallel run of ONE filter over a long event stream (kf_run_stream; the reference's own
// use of run_kalman_filter_full, kf_workers.py:623-728, is one filter over a whole drive log).
// The stream is cut into C chunks of L events that run as filters of the chain kernel:
//  * the covariance recursion does not depend on the measurements and forgets its start, so
//    chunk c's start covariance is the handle's P carried over the chunks before it by their
//    linear-fractional covariance maps (phases 6-7; or an event warm-up over the W events before
//    it, the warm-up bank);
//  * given the gains, the state recursion is affine (the IMU pseudo-measurement is built from
//    the predicted state, kf_workers.py:698-706, which keeps it affine), and block-diagonal
//    over the axis chains: the map pass runs each chunk from a guess and from three perturbed
//    guesses (one per chain component; the four variants share one lane and one covariance),
//    its epilogue giving x_end = A x_start + b per chunk and chain;
//  * the maps are composed from the handle's state by a parallel scan (phases 2-4) into every
//    chunk's true start; the records are the map pass's, the trajectory evaluated at the true
//    starts (phase 8), or a final pass runs the chunks from them (KF_OPT_STREAM_FINAL = 1);
//  * checks: each chunk's start covariance equals the previous chunk's end covariance, the
//    starts and the end state are finite (a final pass: each chunk's end state is its
//    successor's start), no chunk filter failed.  Only then does the handle take the end
//    state; otherwise the sequential chain kernel, launched after these with skip = &check.ok,
//    runs the stream as one filter and rewrites every record.
// ------------------------------------------------------------------------------------
#ifndef KF_STREAM_RECORD_PAIRS
#define KF_STREAM_RECORD_PAIRS 1
#endif
// the records from the map pass two entries per thread (stream_records2_kernel; 0: one each)
constexpr bool kStreamRecordPairs = KF_STREAM_RECORD_PAIRS != 0;

template <class M>
__device__ __forceinline__ int chain_state(int a, int q) {  // chain a (pva chains first), component q; -1: none
    return a < M::NP ? M::pva(a, q) : (q < 2 ? M::aw(a - M::NP, q) : -1);
}
template <class M>
__device__ __forceinline__ int chain_row0(int a) {  // first block-packed covariance row of chain a
    return a < M::NP ? 6 * a : 6 * M::NP + 3 * (a - M::NP);
}
template <class M>
__device__ __forceinline__ int state_component(int i) {  // component of state i within its chain
    int comp = 0;
#pragma unroll
    for (int a = 0; a < M::NP + M::NA; ++a)
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (chain_state<M>(a, q) == i) comp = q;
    return comp;
}

// phase 0: every chunk of the warm-up bank starts from the handle's state; check zeroed
template <typename T, class M>
__global__ __launch_bounds__(kBlock) void stream_init_kernel(const StreamArgs a) {
    const int64_t c = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (c == 0) {
        a.check->ok = 0;
        a.check->bad = 0;
        a.check->cov_gap = 0.0;
        a.check->state_gap = 0.0;
        a.check->done = 0;
        a.check->skip_chain = 0;
    }
    if (c >= a.C) return;
    const T* hx = static_cast<const T*>(a.hx);
    const T* hP = static_cast<const T*>(a.hP);
#pragma unroll
    for (int i = 0; i < M::N; ++i) static_cast<T*>(a.wx)[i * a.C + c] = hx[i];
#pragma unroll
    for (int r = 0; r < M::NBLK; ++r) static_cast<T*>(a.wP)[r * a.C + c] = hP[r];
    a.wst[c] = a.hstatus[0];
}

// phase 1: map bank filter q * C + c = chunk c from its warm-up state, + delta on component q - 1
// of every chain (q = 0: the guess itself)
template <typename T, class M>
__global__ __launch_bounds__(kBlock) void stream_perturb_kernel(const StreamArgs a) {
    const int64_t f = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    const int64_t B = 4 * a.C;
    if (f >= B) return;
    const int q = int(f / a.C);
    const int64_t c = f % a.C;
#pragma unroll
    for (int i = 0; i < M::N; ++i) {
        const T g = static_cast<const T*>(a.wx)[i * a.C + c];
        static_cast<T*>(a.mx)[i * B + f] = (q > 0 && state_component<M>(i) == q - 1) ? g + T(a.delta) : g;
    }
#pragma unroll
    for (int r = 0; r < M::NBLK; ++r) static_cast<T*>(a.mP)[r * B + f] = static_cast<const T*>(a.wP)[r * a.C + c];
    a.mst[f] = a.wst[c];
}

template <class M>
__device__ __forceinline__ void compose_into(double (&A)[3][3], double (&b)[3], const double* m) {
    // (A, b) <- m o (A, b): A = Am A, b = Am b + bm
    double An[3][3], bn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double t = m[9 + k];
#pragma unroll
        for (int q = 0; q < 3; ++q) t = __builtin_fma(m[k * 3 + q], b[q], t);
        bn[k] = t;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double u = 0.0;
#pragma unroll
            for (int q = 0; q < 3; ++q) u = __builtin_fma(m[k * 3 + q], A[q][j], u);
            An[k][j] = u;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        b[k] = bn[k];
#pragma unroll
        for (int j = 0; j < 3; ++j) A[k][j] = An[k][j];
    }
}
__device__ __forceinline__ void apply_map(double (&x)[3], const double* m) {
    double xn[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double t = m[9 + k];
#pragma unroll
        for (int q = 0; q < 3; ++q) t = __builtin_fma(m[k * 3 + q], x[q], t);
        xn[k] = t;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) x[k] = xn[k];
}

// phases 2-4: the chunk maps (written by the map pass's epilogue) composed into every chunk's
// true start, as a three-kernel parallel scan per chain (a dependent walk over the maps waits
// ~1 us per map load):
//   2  tiles of kScanTile chunks: thread c loads chunk c's map, a Kogge-Stone scan in LDS gives
//      its exclusive in-tile prefix E_c (stored) and the tile's product (stored);
//   3  one block per chain: the same scan over the tile products (rounds of kScanTile tiles with a
//      carry) applied to the handle's state gives every tile's start, and the stream's end state;
//   4  thread per (chunk, chain): start = E_c(tile start), stored (before a final pass also the
//      final bank's state, covariance and status) and checked finite.  The last block to finish
//      (a counter; release / acquire fences) gives the verdict when the records come from the map
//      pass (a.xend): no failed chunk filter, finite starts and end state, covariance seams within
//      tolerance; a passed run leaves the end state and the last chunk's end covariance in the
//      handle.  No state seam is measured there (the starts are the maps' values, not runs from
//      them; KF_OPT_STREAM_FINAL = 1 runs them and checks the seams in phase 5).
constexpr int kScanTile = 256;
__device__ __forceinline__ void affine_compose(double (&o)[12], const double (&l)[12], const double (&e)[12]) {
    // o = l o e: A = A_l A_e, b = A_l b_e + b_l
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        double t = l[9 + k];
#pragma unroll
        for (int q = 0; q < 3; ++q) t = __builtin_fma(l[k * 3 + q], e[9 + q], t);
        o[9 + k] = t;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double u = 0.0;
#pragma unroll
            for (int q = 0; q < 3; ++q) u = __builtin_fma(l[k * 3 + q], e[q * 3 + j], u);
            o[k * 3 + j] = u;
        }
    }
}

__device__ __forceinline__ void affine_identity(double (&m)[12]) {
#pragma unroll
    for (int e = 0; e < 12; ++e) m[e] = (e == 0 || e == 4 || e == 8) ? 1.0 : 0.0;
}

// Inclusive Kogge-Stone scan of one affine map per thread over the block (LDS, struct of
// arrays): v <- v_t o ... o v_0.  The caller syncs before reusing `pre`.
__device__ __forceinline__ void block_scan_affine(double (&v)[12], double (*pre)[kScanTile], int tid) {
#pragma unroll
    for (int e = 0; e < 12; ++e) pre[e][tid] = v[e];
    __syncthreads();
    for (int d = 1; d < kScanTile; d <<= 1) {
        double earlier[12];
        const bool has = tid >= d;
        if (has) {
#pragma unroll
            for (int e = 0; e < 12; ++e) earlier[e] = pre[e][tid - d];
        }
        __syncthreads();
        if (has) {
            double o[12];
            affine_compose(o, v, earlier);
#pragma unroll
            for (int e = 0; e < 12; ++e) {
                v[e] = o[e];
                pre[e][tid] = o[e];
            }
        }
        __syncthreads();
    }
}

// phase 2: grid (tiles, chains)
template <typename T, class M>
__global__ __launch_bounds__(kScanTile) void stream_scan_tiles_kernel(const StreamArgs a) {
    constexpr int NCH = M::NP + M::NA;
    __shared__ double pre[12][kScanTile];
    const int tid = int(threadIdx.x);
    const int ch = int(blockIdx.y);
    const int64_t tile = blockIdx.x, c = tile * kScanTile + tid;
    double v[12];
    if (c < a.C) {
#pragma unroll
        for (int e = 0; e < 12; ++e) v[e] = a.maps[(c * NCH + ch) * 12 + e];
    } else {
        affine_identity(v);
    }
    block_scan_affine(v, pre, tid);
    if (c < a.C) {
        double* o = a.pref + (c * NCH + ch) * 12;
        if (tid == 0) {
            double id[12];
            affine_identity(id);
#pragma unroll
            for (int e = 0; e < 12; ++e) o[e] = id[e];
        } else {
#pragma unroll
            for (int e = 0; e < 12; ++e) o[e] = pre[e][tid - 1];
        }
    }
    if (tid == kScanTile - 1) {
        double* o = a.tiles + (tile * NCH + ch) * 12;
#pragma unroll
        for (int e = 0; e < 12; ++e) o[e] = v[e];
    }
}

// phase 3 (only when there are more tiles than one scan round holds): grid (1, chains).  The
// scan's top phase as a launch of its own: rounds of kScanTile tile products, each scanned and
// applied to the carried state, give every tile's start state in a.tstart.  Below that size
// the starts kernel composes its own prefix (one round per block, no launch).
template <typename T, class M>
__global__ __launch_bounds__(kScanTile) void stream_top_kernel(const StreamArgs a) {
    constexpr int NCH = M::NP + M::NA;
    __shared__ double pre[12][kScanTile];
    __shared__ double carry[3];
    const int tid = int(threadIdx.x);
    const int ch = int(blockIdx.y);
    const int ns = ch < M::NP ? 3 : 2;
    const int64_t ntiles = (a.C + kScanTile - 1) / kScanTile;
    if (tid < 3) carry[tid] = tid < ns ? double(static_cast<const T*>(a.hx)[chain_state<M>(ch, tid)]) : 0.0;
    for (int64_t r0 = 0; r0 < ntiles; r0 += kScanTile) {
        const int64_t t = r0 + tid;
        double v[12];
        if (t < ntiles) {
#pragma unroll
            for (int e = 0; e < 12; ++e) v[e] = a.tiles[(t * NCH + ch) * 12 + e];
        } else {
            affine_identity(v);
        }
        __syncthreads();  // carry written (the previous round / the init), pre free
        block_scan_affine(v, pre, tid);
        if (t < ntiles) {  // tile t's start: the round's carry through the tiles before t
            double x[3] = {carry[0], carry[1], carry[2]};
            if (tid > 0) {
                double e1[12];
#pragma unroll
                for (int e = 0; e < 12; ++e) e1[e] = pre[e][tid - 1];
                apply_map(x, e1);
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) a.tstart[(t * NCH + ch) * 3 + k] = x[k];
        }
        __syncthreads();  // every thread has read carry and pre
        if (tid == kScanTile - 1) {  // the round's product (identity maps past the last tile)
            double xe[3] = {carry[0], carry[1], carry[2]};
            apply_map(xe, v);
#pragma unroll
            for (int k = 0; k < 3; ++k) carry[k] = xe[k];
        }
    }
}

// phase 4: grid (tiles, chains).  Each block first composes the products of the tiles before
// its own into its tile start — at most one round of kScanTile tiles; with more tiles the top
// kernel (phase 3) has written every tile start to a.tstart, since redoing the prefix per block
// would cost O(ntiles^2) — and the block of the last tile also runs through its own
// product: the stream's end state.
template <typename T, class M>
__global__ __launch_bounds__(kScanTile) void stream_starts_kernel(const StreamArgs a) {
    constexpr int NCH = M::NP + M::NA;
    __shared__ double pre[12][kScanTile];
    __shared__ double carry[3];
    const int tid = int(threadIdx.x);
    const int ch = int(blockIdx.y);
    const int ns = ch < M::NP ? 3 : 2;
    const int64_t tile = blockIdx.x, c = tile * kScanTile + tid;
    const int64_t ntiles = gridDim.x;
    if (a.tstart) {
        if (tid < 3) carry[tid] = tid < ns ? a.tstart[(tile * NCH + ch) * 3 + tid] : 0.0;
    } else if (tid < 3) {
        carry[tid] = tid < ns ? double(static_cast<const T*>(a.hx)[chain_state<M>(ch, tid)]) : 0.0;
    }
    for (int64_t r0 = 0; !a.tstart && r0 < tile; r0 += kScanTile) {
        const int64_t t = r0 + tid;
        double v[12];
        if (t < tile) {
#pragma unroll
            for (int e = 0; e < 12; ++e) v[e] = a.tiles[(t * NCH + ch) * 12 + e];
        } else {
            affine_identity(v);
        }
        __syncthreads();  // carry written (the previous round / the init), pre free
        block_scan_affine(v, pre, tid);
        if (tid == kScanTile - 1) {  // the round's product (identity maps past `tile`)
            double xe[3] = {carry[0], carry[1], carry[2]};
            apply_map(xe, v);
#pragma unroll
            for (int k = 0; k < 3; ++k) carry[k] = xe[k];
        }
    }
    __syncthreads();
    bool fin = true;
    if (a.xend && tile == ntiles - 1 && tid == 0) {  // the stream's end state
        double xe[3] = {carry[0], carry[1], carry[2]}, tp[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) tp[e] = a.tiles[(tile * NCH + ch) * 12 + e];
        apply_map(xe, tp);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k >= ns) continue;
            // read by the verdict's block (maybe on another XCD): a device-scope atomic
            atomicExch(reinterpret_cast<unsigned long long*>(&a.xend[chain_state<M>(ch, k)]),
                       static_cast<unsigned long long>(__double_as_longlong(xe[k])));
            fin = fin && (xe[k] - xe[k] == 0.0);
        }
    }
    if (c < a.C) {
        double x[3] = {carry[0], carry[1], carry[2]}, e1[12];
#pragma unroll
        for (int e = 0; e < 12; ++e) e1[e] = a.pref[(c * NCH + ch) * 12 + e];
        apply_map(x, e1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k >= ns) continue;
            const int i = chain_state<M>(ch, k);
            a.starts[i * a.C + c] = x[k];
            // the records' offsets, start - guess, in the records kernel's own arithmetic
            if (a.dtab) a.dtab[(c * NCH + ch) * 4 + k] = x[k] - double(static_cast<const T*>(a.wx)[i * a.C + c]);
            fin = fin && (x[k] - x[k] == 0.0);  // NaN or inf fails
            if (!a.xend) static_cast<T*>(a.fx)[i * a.C + c] = T(x[k]);
        }
        if (!a.xend) {  // the final bank: the warm-up covariance, status 0
            const int r0 = chain_row0<M>(ch), nr = ns == 3 ? 6 : 3;
            for (int r = r0; r < r0 + nr; ++r)
                static_cast<T*>(a.fP)[r * a.C + c] = static_cast<const T*>(a.wP)[r * a.C + c];
            if (ch == 0) a.fst[c] = 0;
        }
    }
    const bool all_fin = __syncthreads_and(fin ? 1 : 0) != 0;
    if (tid != 0) return;
    StreamCheck* k = a.check;
    if (!all_fin) atomicOr(&k->bad, kStreamBadStart);
    if (!a.xend) return;  // a final pass follows: phase 5 decides
    // Everything the verdict reads from this launch travels by device-scope atomics (bad here,
    // cov_gap and bad from the map pass and the end state from earlier launches), so no fence:
    // the wave only drains its own atomic before it counts itself (an agent-scope release per
    // block wrote its XCD's L2 back and cost more than the kernel's work).  The empty asm with a
    // memory clobber keeps the compiler from moving the bad update past the count (s_waitcnt
    // alone is not a compiler barrier); the wait then drains it in the hardware.
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_waitcnt(0);
    const int blocks = int(gridDim.x * gridDim.y);
    if (atomicAdd(&k->done, 1) != blocks - 1) return;
    asm volatile("" ::: "memory");  // the verdict's reads stay after the count
    const int bad = atomicOr(&k->bad, 0);
    const double cov_gap = __longlong_as_double(atomicOr(reinterpret_cast<unsigned long long*>(&k->cov_gap), 0ull));
    const bool ok = bad == 0 && cov_gap <= a.tol_cov;
    // every read issued before the first store: a read after a store that may alias it waits
    // for the store, which made the 42 reads below round trips one after another
    const int64_t col = a.C - 1, B4 = 4 * a.C;  // the last chunk's end covariance
    double xv[M::N];
    T pv[M::NBLK];
    if (ok) {
#pragma unroll
        for (int i = 0; i < M::N; ++i)  // written by the last tile's block (a device-scope atomic)
            xv[i] = __longlong_as_double(
                static_cast<long long>(atomicOr(reinterpret_cast<unsigned long long*>(&a.xend[i]), 0ull)));
#pragma unroll
        for (int r = 0; r < M::NBLK; ++r) pv[r] = static_cast<const T*>(a.mP)[r * B4 + col];
    }
    k->state_gap = bad & kStreamBadStart ? __builtin_inf() : __builtin_nan("");
    k->ok = ok ? 1 : 0;
    if (ok) {
#pragma unroll
        for (int i = 0; i < M::N; ++i) static_cast<T*>(a.hx)[i] = T(xv[i]);
#pragma unroll
        for (int r = 0; r < M::NBLK; ++r) static_cast<T*>(a.hP)[r] = pv[r];
        a.hstatus[0] = 0;
    }
}

// phase 8 (records from the map pass): thread per (event, trajectory entry i); entry i (the
// first component of its chain) = variant 0's + sum_q A_q (start - guess)_q with A_q =
// (variant q+1 - variant 0) / delta, as the chunk maps
template <typename T, class M>
__global__ __launch_bounds__(kBlock) void stream_records_kernel(const StreamArgs a) {
    constexpr int NCH = M::NP + M::NA;
    const int64_t g = int64_t(blockIdx.x) * kBlock + threadIdx.x;  // e * NTRAJ + i: coalesced rows
    if (g >= a.S * M::NTRAJ) return;
    // 32-bit divisions (S * NTRAJ < 2^31: kf_run_stream's offsets are 32-bit)
    const uint32_t e = uint32_t(g) / uint32_t(M::NTRAJ);
    const int i = int(uint32_t(g) - e * uint32_t(M::NTRAJ));
    const int64_t c = e / uint32_t(a.L);
    const T* t4 = static_cast<const T*>(a.traj4);
    const T* wx = static_cast<const T*>(a.wx);
    int ch = 0;  // the chain whose first component is state i (the trajectory holds those)
#pragma unroll
    for (int cc = 0; cc < NCH; ++cc)
        if (chain_state<M>(cc, 0) == i) ch = cc;
    const int ns = ch < M::NP ? 3 : 2;
    const double x0 = double(t4[g]);
    double acc = x0;
    // start - guess of the chain's components: the starts kernel's table (two loads shared by
    // the chunk's threads), or the starts and guess rows themselves
    double d[3];
    if (a.dtab) {
        const double* dt = a.dtab + (c * NCH + ch) * 4;
        const double2 d01 = *reinterpret_cast<const double2*>(dt);
        d[0] = d01.x;
        d[1] = d01.y;
        d[2] = ns == 3 ? dt[2] : 0.0;
    } else {
#pragma unroll
        for (int qq = 0; qq < 3; ++qq) {
            const int idx = chain_state<M>(ch, qq);
            d[qq] = qq < ns ? a.starts[idx * a.C + c] - double(wx[idx * a.C + c]) : 0.0;
        }
    }
#pragma unroll
    for (int qq = 0; qq < 3; ++qq) {
        if (qq >= ns) continue;
        const double xq = double(t4[(qq + 1) * a.vstride * M::NTRAJ + g]);
        acc = __builtin_fma((xq - x0) * a.rdelta, d[qq], acc);  // delta is a power of two: exact
    }
    static_cast<T*>(a.traj)[g] = T(acc);
}

// The same records two entries per thread (an even NTRAJ: entries 2j, 2j + 1 of one event):
// one 2-wide load per variant row and one 2-wide store instead of two each, the start offsets
// from the starts kernel's table.  Each entry's arithmetic is stream_records_kernel's.
template <typename T, class M>
__global__ __launch_bounds__(kBlock) void stream_records2_kernel(const StreamArgs a) {
    static_assert(M::NTRAJ % 2 == 0, "pairs of one event's entries");
    typedef T T2 __attribute__((ext_vector_type(2)));
    constexpr int NCH = M::NP + M::NA;
    const int64_t p = int64_t(blockIdx.x) * kBlock + threadIdx.x;  // pair: entries 2p, 2p + 1
    if (p >= a.S * (M::NTRAJ / 2)) return;
    const uint32_t e = uint32_t(p) / uint32_t(M::NTRAJ / 2);
    const int i0 = 2 * int(uint32_t(p) - e * uint32_t(M::NTRAJ / 2));
    const int64_t c = e / uint32_t(a.L);
    const T2* t4 = static_cast<const T2*>(a.traj4);
    int ch[2] = {0, 0};
#pragma unroll
    for (int cc = 0; cc < NCH; ++cc) {
        if (chain_state<M>(cc, 0) == i0) ch[0] = cc;
        if (chain_state<M>(cc, 0) == i0 + 1) ch[1] = cc;
    }
    double d[2][3];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const double* dt = a.dtab + (c * NCH + ch[h]) * 4;
        const double2 d01 = *reinterpret_cast<const double2*>(dt);
        d[h][0] = d01.x;
        d[h][1] = d01.y;
        d[h][2] = ch[h] < M::NP ? dt[2] : 0.0;
    }
    const T2 v0 = t4[p];
    const double x0[2] = {double(v0.x), double(v0.y)};
    double acc[2] = {x0[0], x0[1]};
    const bool any3 = ch[0] < M::NP || ch[1] < M::NP;  // a third variant row is needed
#pragma unroll
    for (int qq = 0; qq < 3; ++qq) {
        if (qq == 2 && !any3) continue;
        const T2 vq = t4[(qq + 1) * a.vstride * (M::NTRAJ / 2) + p];
        const double xq[2] = {double(vq.x), double(vq.y)};
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int ns = ch[h] < M::NP ? 3 : 2;
            if (qq < ns) acc[h] = __builtin_fma((xq[h] - x0[h]) * a.rdelta, d[h][qq], acc[h]);
        }
    }
    T2 out;
    out.x = T(acc[0]);
    out.y = T(acc[1]);
    static_cast<T2*>(a.traj)[p] = out;
}

// ------------------------------------------------------------------------------------
// Covariance warm-up by linear-fractional maps (kf_run_stream's default).  Per axis chain the
// covariance recursion is P <- (A P + B)(C P + D)^-1 with, per event,
//   predict  [[F, Q F^-T], [0, F^-T]]      (F P F^T + Q with P = X Y^-1)
//   update   [[I, 0], [H^T R^-1 H, I]]     ((P^-1 + H^T R^-1 H)^-1, the Joseph form's value)
// so a chunk's covariance map is the 6x6 product of its events' matrices (an (att, rate)
// chain carries the chain kernel's inert third state as an identity row and column).  The
// chunk starts are then the fixed point of P(c) = map_(c-1)(P(c-1)) from P(0) = the handle's
// P, reached by parallel iterations: the recursion forgets its start (each chunk of the
// reference's 200 Hz IMU stream contracts an error by ~1e-3), so a few iterations over all
// chunks at once replace the W-event warm-up; the device seam check still decides.
// ------------------------------------------------------------------------------------
// ChainLane's noise table restated for the maps: fp64 whatever T is, R as reciprocals, and the
// inert third state of an aw chain without a measurement (1 / R = 0) where the event has R = 1
template <class M, bool CUSTOM>
__device__ __forceinline__ void chain_noise(int ch, double (&q)[3], double (&si_imu)[3], double& si_gps,
                                            const RefConsts* kc) {
    const bool pva = ch < M::NP;
    if constexpr (CUSTOM) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int i = chain_state<M>(ch, k);
            q[k] = i >= 0 ? ro(kc)->q[i] : 0.0;
            si_imu[k] = i >= 0 ? 1.0 / ro(kc)->r_imu[i] : 0.0;
        }
        si_gps = pva ? 1.0 / ro(kc)->r_gps[ch] : 0.0;
        return;
    }
    q[0] = pva ? kQPos : kQAtt;
    q[1] = pva ? kQVel : kQRate;
    q[2] = pva ? kQAcc : 0.0;
    si_imu[0] = 1.0 / (pva ? kRPos : kRAtt);
    si_imu[1] = 1.0 / (pva ? kRVel : kRRate);
    si_imu[2] = pva ? 1.0 / kRAcc : 0.0;
    si_gps = pva ? 1.0 / kRGps : 0.0;
}

// phase 6: the product of each chunk piece's event matrices per chain, one lane per (piece,
// chain) holding the 6x6 product (an event acts on its columns independently).  Rescaled by a
// power of two (the product's max) every 16 events, which a linear-fractional map ignores.
// Event types and dt are loaded 8 events at a time, one batch ahead.
template <class M>
__device__ __forceinline__ void lft_event(double (&v)[6], int type, double dt, bool pva, const double (&q)[3],
                                          const double (&si)[3], double sg) {
    if (type == 255) return;
    const double c02 = pva ? 0.5 * dt * dt : 0.0, c12 = pva ? dt : 0.0;
    const double g20 = dt * c12 - c02;
    // bottom <- F^-T bottom; top <- F top + Q dt (new bottom)
    const double b0 = v[3], b1 = __builtin_fma(-dt, v[3], v[4]);
    const double b2 = __builtin_fma(g20, v[3], __builtin_fma(-c12, v[4], v[5]));
    const double t0 = __builtin_fma(c02, v[2], __builtin_fma(dt, v[1], v[0]));
    const double t1 = __builtin_fma(c12, v[2], v[1]);
    v[0] = __builtin_fma(q[0] * dt, b0, t0);
    v[1] = __builtin_fma(q[1] * dt, b1, t1);
    v[2] = __builtin_fma(q[2] * dt, b2, v[2]);
    v[3] = b0;
    v[4] = b1;
    v[5] = b2;
    if (type == kGps || type == kImu) {  // bottom += H^T R^-1 H top
        const bool gps = type == kGps;
        v[3] = __builtin_fma(gps ? sg : si[0], v[0], v[3]);
        v[4] = __builtin_fma(gps ? 0.0 : si[1], v[1], v[4]);
        v[5] = __builtin_fma(gps ? 0.0 : si[2], v[2], v[5]);
    }
}

// kLftHalves lanes per (chunk piece, chain), each carrying 6 / kLftHalves columns of the 6x6
// product: the columns are independent, so the split multiplies the waves of this latency-bound
// pass (0.75 wave per SIMD at 8192 chunks with all six columns in one lane) at the cost of
// paying an event's type / dt handling in every lane.  Config 1 in-process, with the axis-
// symmetric maps: 1 / 2 / 3 / 6 lanes 0.208 / 0.200 / 0.195 / 0.196 ms per log
// (profiles/r04_pmc/cfg1_diag/ab_halves.log)
#ifndef KF_LFT_HALVES
#define KF_LFT_HALVES 3
#endif
constexpr int kLftHalves = KF_LFT_HALVES;
static_assert(6 % kLftHalves == 0, "columns per lane");
// lanes per product: a power of two for the max exchange (3 / 6 column lanes: one / two lanes
// duplicate the last column and store nothing)
constexpr int kLftStride = kLftHalves == 3 ? 4 : kLftHalves == 6 ? 8 : kLftHalves;
// a.sym: the maps of chains 0 (pva) and NP (aw) only, which stand for every chain
template <class M>
__host__ __device__ constexpr int lft_map_chains(bool sym) {
    return sym ? 1 + (M::NA > 0 ? 1 : 0) : M::NP + M::NA;
}
template <class M>
__device__ __forceinline__ int lft_map_chain(bool sym, int ch) {  // whose maps chain ch uses
    return sym ? (ch < M::NP ? 0 : M::NP) : ch;
}
template <typename T, class M, bool CUSTOM>
__global__ __launch_bounds__(kBlock) void stream_lft_maps_kernel(const StreamArgs a) {
    constexpr int NCH = M::NP + M::NA;
    constexpr int NJ = 6 / kLftHalves;  // columns per lane
    const int nmc = lft_map_chains<M>(a.sym != 0);
    const int64_t gl = int64_t(blockIdx.x) * kBlock + threadIdx.x;
    if (gl >= a.C * a.np * nmc * kLftStride) return;  // whole products (kLftStride divides the wave)
    const int64_t gm = gl / kLftStride;  // (chunk * np + piece) * nmc + map chain
    const int li = int(gl % kLftStride);
    const bool own = li < kLftHalves;
    const int j0 = (own ? li : kLftHalves - 1) * NJ;
    const int64_t cp = gm / nmc;  // chunk * np + piece
    const int cm = int(gm % nmc);
    const int ch = a.sym ? (cm == 0 ? 0 : M::NP) : cm;
    const int64_t grp = cp * NCH + ch;  // the map's slot
    const bool pva = ch < M::NP;
    double q[3], si[3], sg;
    chain_noise<M, CUSTOM>(ch, q, si, sg, a.kc);
    double v[NJ][6];  // v[j] = column j0 + j
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int i = 0; i < 6; ++i) v[j][i] = i == j0 + j ? 1.0 : 0.0;
    const int64_t c = cp / a.np, piece = cp % a.np;
    const int64_t cend = (c + 1) * a.L < a.S ? (c + 1) * a.L : a.S;
    const int64_t e0 = c * a.L + piece * a.lp, e1 = e0 + a.lp < cend ? e0 + a.lp : cend;
    // events in batches of 8, the next batch's type and dt loaded while this one computes.  The
    // loads are unconditional buffer loads (past the stream they return 0) and the batch's range
    // test is applied where the values are used: loads under a per-lane condition were branched
    // around, and the branches' join waited for every load in flight (vmcnt 0), the batch just
    // issued included
    constexpr int kB = 8;
    const auto r_et = bytes_rsrc(a.etype, uint32_t(a.S));
    const auto r_dt = bytes_rsrc(a.dt, uint32_t(a.S) * 8u);
    uint32_t tyn[kB];
    double dvn[kB];
    auto fetch = [&](int64_t e) {
#pragma unroll
        for (int k = 0; k < kB; ++k) {
            const uint32_t ue = uint32_t(e + k);
            tyn[k] = __builtin_amdgcn_raw_buffer_load_b8(r_et, ue, 0, 0);
            dvn[k] = ldv(r_dt, ue * 8u, 0.0);
        }
    };
    fetch(e0);
    for (int64_t e = e0; e < e1; e += kB) {
        uint32_t ty[kB];
        double dv[kB];
#pragma unroll
        for (int k = 0; k < kB; ++k) {
            ty[k] = tyn[k];
            dv[k] = dvn[k];
        }
        fetch(e + kB);
#pragma unroll
        for (int k = 0; k < kB; ++k) {
            const bool in = e + k < e1;
            const int tk = in ? int(ty[k]) : 255;
            const double dk = in ? dv[k] : 0.0;
#pragma unroll
            for (int j = 0; j < NJ; ++j) lft_event<M>(v[j], tk, dk, pva, q, si, sg);
        }
        if (((e - e0) & 15) == kB) {  // every 16 events: rescale by a power of two (the max)
            // of all six columns: the lanes of one product exchange their maxima (adjacent lanes)
            double mx = 0.0;
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int i = 0; i < 6; ++i) mx = fmax(mx, fabs(v[j][i]));
#pragma unroll
            for (int sh = 1; sh < kLftStride; sh <<= 1) mx = fmax(mx, __shfl_xor(mx, sh, 64));
            int ex;
            (void)frexp(mx, &ex);
            const double sc = ldexp(1.0, -ex);
#pragma unroll
            for (int j = 0; j < NJ; ++j)
#pragma unroll
                for (int i = 0; i < 6; ++i) v[j][i] *= sc;
        }
    }
    if (!own) return;
    double* o = a.phi + grp * 36;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) o[i * 6 + j0 + j] = v[j][i];
}

// a chain's block of the block-packed covariance as a full 3x3 (the inert state: variance 1)
template <typename T, class M>
__device__ __forceinline__ void chain_block_full(const T* P, int64_t stride, int64_t col, int ch, double (&p)[3][3]) {
    const int r0 = chain_row0<M>(ch);
    if (ch < M::NP) {
        const double v[6] = {double(P[(r0 + 0) * stride + col]), double(P[(r0 + 1) * stride + col]),
                             double(P[(r0 + 2) * stride + col]), double(P[(r0 + 3) * stride + col]),
                             double(P[(r0 + 4) * stride + col]), double(P[(r0 + 5) * stride + col])};
        p[0][0] = v[0], p[0][1] = p[1][0] = v[1], p[0][2] = p[2][0] = v[2];
        p[1][1] = v[3], p[1][2] = p[2][1] = v[4], p[2][2] = v[5];
    } else {
        const double v[3] = {double(P[(r0 + 0) * stride + col]), double(P[(r0 + 1) * stride + col]),
                             double(P[(r0 + 2) * stride + col])};
        p[0][0] = v[0], p[0][1] = p[1][0] = v[1], p[1][1] = v[2];
        p[0][2] = p[2][0] = p[1][2] = p[2][1] = 0.0;
        p[2][2] = 1.0;
    }
}

// one piece map applied to a chain covariance p (3x3, in place): P' = X Y^-1 with
// [X; Y] = [[A, B], [C, D]] [P; I], via the adjugate of Y, then symmetrised
__device__ __forceinline__ void lft_apply(double (&p)[3][3], const double (&m)[36]) {
    double X[3][3], Y[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double x = m[i * 6 + 3 + j], y = m[(i + 3) * 6 + 3 + j];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                x = __builtin_fma(m[i * 6 + k], p[k][j], x);
                y = __builtin_fma(m[(i + 3) * 6 + k], p[k][j], y);
            }
            X[i][j] = x;
            Y[i][j] = y;
        }
    const double a00 = Y[1][1] * Y[2][2] - Y[1][2] * Y[2][1], a01 = Y[0][2] * Y[2][1] - Y[0][1] * Y[2][2],
                 a02 = Y[0][1] * Y[1][2] - Y[0][2] * Y[1][1];
    const double a10 = Y[1][2] * Y[2][0] - Y[1][0] * Y[2][2], a11 = Y[0][0] * Y[2][2] - Y[0][2] * Y[2][0],
                 a12 = Y[0][2] * Y[1][0] - Y[0][0] * Y[1][2];
    const double a20 = Y[1][0] * Y[2][1] - Y[1][1] * Y[2][0], a21 = Y[0][1] * Y[2][0] - Y[0][0] * Y[2][1],
                 a22 = Y[0][0] * Y[1][1] - Y[0][1] * Y[1][0];
    const double det = Y[0][0] * a00 + Y[0][1] * a10 + Y[0][2] * a20;
    const double inv[3][3] = {{a00, a01, a02}, {a10, a11, a12}, {a20, a21, a22}};
    const double rd = rcp_nr<2>(det);  // Newton-refined reciprocal: an IEEE division is ~10 dependent ops
    double pn[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s = __builtin_fma(X[i][k], inv[k][j], s);
            pn[i][j] = s * rd;
        }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i + 1; j < 3; ++j) pn[i][j] = pn[j][i] = 0.5 * (pn[i][j] + pn[j][i]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) p[i][j] = pn[i][j];
}

// phase 7: every chunk's start covariance from the maps, in ONE launch: chunk c starts from the
// handle's P advanced by the piece maps of at least the `iters` chunks before it (every chunk
// from the stream start when c < iters: exact), which covers the recursion's forgetting.  Block
// (x, chain) owns chunks [b0, b0 + a.G) of one chain, a.g consecutive chunks per thread: its
// threads first stage every piece map the windows need, [max(0, b0 - iters), b0 + G - 1) x np,
// into LDS (struct of arrays) with coalesced loads (a dependent walk over global memory waited
// ~2 us per map), then thread t walks from max(0, c_t - iters) through its g chunks, recording
// each start: (iters + g - 1) maps for g chunks.  a.g = 0: no LDS (windows too long for it), one
// chunk per thread, maps read from global memory.  For every chunk it also writes the warm-up
// bank (the handle's state as the guess, its status) and, without event warm-up (a.kp == 0),
// the map bank itself: every variant's covariance column (the map pass reads column c) and the
// guesses, variant q + 1 with + delta on component q of every chain.  Thread 0 of block 0
// zeroes the check.
constexpr int kStartMaxG = 4;  // chunks per thread of the start kernel (their starts stay in registers)
// NU: the LDS maps' row pitch fixed at compile time (where the block's window maps fit it): a
// walk's 36 reads of a map are then immediate offsets from one address, where a runtime pitch
// cost an address add per element and the products of each chunk's rows (~120 of the ~290
// instructions of a map application)
constexpr int kStartNu = 192;
template <typename T, class M, bool LDS, bool NU = false>
__global__ __launch_bounds__(kBlock) void stream_lft_start_kernel(const StreamArgs a) {
    extern __shared__ double lmap[];  // [36][nu]: element e of the block's nu = (G + iters) * np window maps
    constexpr int NCH = M::NP + M::NA;
    const int tid = int(threadIdx.x);
    const int ch = int(blockIdx.y);
    if (blockIdx.x == 0 && ch == 0 && tid == 0) {
        a.check->ok = 0;
        a.check->bad = 0;
        a.check->cov_gap = 0.0;
        a.check->state_gap = 0.0;
        a.check->done = 0;
        a.check->skip_chain = 0;
    }
    const int64_t gt = LDS ? a.g : 1;                  // chunks per thread
    const int64_t BC = LDS ? a.G : int64_t(blockDim.x);  // chunks per block
    const int64_t b0 = int64_t(blockIdx.x) * BC;
    const int64_t ws = b0 - a.iters > 0 ? b0 - a.iters : 0;  // first chunk whose maps the block reads
    // struct of arrays: at each step of the walks, consecutive threads read maps g apart
    const uint32_t nu = NU ? uint32_t(kStartNu) : uint32_t((BC + a.iters) * a.np);
    if constexpr (LDS) {
        const int64_t we = (b0 + BC < a.C ? b0 + BC : a.C) - 1;  // maps of chunks [ws, we)
        // 32-bit indices (a 64-bit division is a ~100-instruction sequence per element), 16 loads
        // in flight per thread (a load-store loop waited one memory latency per element)
        const uint32_t n = uint32_t(we > ws ? we - ws : 0) * uint32_t(a.np) * 36u;
        const double* src = a.phi + (ws * a.np * NCH + lft_map_chain<M>(a.sym != 0, ch)) * 36;
        constexpr int kU = 16;
        const uint32_t nt = blockDim.x;
        for (uint32_t e0 = uint32_t(tid); e0 < n; e0 += kU * nt) {
            double v[kU];
#pragma unroll
            for (int j = 0; j < kU; ++j) {
                const uint32_t e = e0 + uint32_t(j) * nt;
                const uint32_t u = e / 36u, k = e - u * 36u;
                v[j] = e < n ? src[u * uint32_t(NCH * 36) + k] : 0.0;
            }
#pragma unroll
            for (int j = 0; j < kU; ++j) {
                const uint32_t e = e0 + uint32_t(j) * nt;
                const uint32_t u = e / 36u, k = e - u * 36u;
                if (e < n) lmap[k * nu + u] = v[j];
            }
        }
        __syncthreads();
    }
    const int64_t ct = b0 + tid * gt;  // this thread's first chunk
    if (ct >= a.C || ct >= b0 + BC) return;
    const int64_t ce = ct + gt < a.C ? ct + gt : a.C;
    const int ns = ch < M::NP ? 3 : 2;
    // every global read before the first store (a load after a store to a pointer that may
    // alias it waits for the store)
    double ph[3][3];
    chain_block_full<T, M>(static_cast<const T*>(a.hP), 1, 0, ch, ph);
    T gx[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) gx[k] = k < ns ? static_cast<const T*>(a.hx)[chain_state<M>(ch, k)] : T(0);
    const int32_t hst = a.hstatus[0];
    double p[3][3], ps[kStartMaxG][3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) p[i][j] = ph[i][j];
    const int64_t cs = ct - a.iters > 0 ? ct - a.iters : 0;
    for (int64_t c = cs; c < ce; ++c) {
        if (c >= ct) {
            const int r = int(c - ct);
#pragma unroll
            for (int rr = 0; rr < kStartMaxG; ++rr)
                if (rr == r)
#pragma unroll
                    for (int i = 0; i < 3; ++i)
#pragma unroll
                        for (int j = 0; j < 3; ++j) ps[rr][i][j] = p[i][j];
        }
        if (c + 1 >= ce) break;
        // chunk c's piece maps in order (each piece short enough for its map to be well
        // conditioned; the LFT error grows with the events one product spans)
        for (int64_t u = c * a.np; u < (c + 1) * a.np; ++u) {
            double m[36];
            if constexpr (LDS) {
                const double* src = lmap + uint32_t(u - ws * a.np);
#pragma unroll
                for (int e = 0; e < 36; ++e) m[e] = src[uint32_t(e) * nu];
            } else {
                const double* src = a.phi + (u * NCH + lft_map_chain<M>(a.sym != 0, ch)) * 36;
#pragma unroll
                for (int e = 0; e < 36; ++e) m[e] = src[e];
            }
            lft_apply(p, m);
        }
    }
    // the starts and the banks; with polish chunks, the warm-up bank runs chunk c + kp from c's
    const int r0 = chain_row0<M>(ch);
    const int64_t B4 = 4 * a.C;
    auto put = [&](T* P, int64_t stride, int64_t col, const double (&q)[3][3]) {
        if (ch < M::NP) {
            P[(r0 + 0) * stride + col] = T(q[0][0]);
            P[(r0 + 1) * stride + col] = T(q[0][1]);
            P[(r0 + 2) * stride + col] = T(q[0][2]);
            P[(r0 + 3) * stride + col] = T(q[1][1]);
            P[(r0 + 4) * stride + col] = T(q[1][2]);
            P[(r0 + 5) * stride + col] = T(q[2][2]);
        } else {
            P[(r0 + 0) * stride + col] = T(q[0][0]);
            P[(r0 + 1) * stride + col] = T(q[0][1]);
            P[(r0 + 2) * stride + col] = T(q[1][1]);
        }
    };
#pragma unroll
    for (int r = 0; r < kStartMaxG; ++r) {
        const int64_t c = ct + r;
        if (c >= ce) break;
        if (c + a.kp < a.C) put(static_cast<T*>(a.wP), a.C, c + a.kp, ps[r]);
        if (c < a.kp) put(static_cast<T*>(a.wP), a.C, c, ph);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (k < ns) static_cast<T*>(a.wx)[chain_state<M>(ch, k) * a.C + c] = gx[k];
        if (ch == 0) a.wst[c] = hst;
        if (a.kp == 0) {
            put(static_cast<T*>(a.mP), B4, c, ps[r]);
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if (k < ns)
                        static_cast<T*>(a.mx)[chain_state<M>(ch, k) * B4 + q * a.C + c] =
                            (q > 0 && k == q - 1) ? gx[k] + T(a.delta) : gx[k];
            if (ch == 0) a.mst[c] = hst;
        }
    }
}

// phase 4 (one block): the state seams and the verdict; a passed run leaves the last chunk's
// end state in the handle
template <typename T, class M>
__global__ __launch_bounds__(1024) void stream_finish_kernel(const StreamArgs a) {
    __shared__ double red[1024];
    __shared__ int redb[1024];
    const int tid = int(threadIdx.x);
    const T* fx = static_cast<const T*>(a.fx);
    double gap = 0.0;
    int bad = 0;
    for (int64_t c = tid; c < a.C; c += blockDim.x) {
        bad |= a.fst[c];
        if (c + 1 < a.C) {
#pragma unroll
            for (int i = 0; i < M::N; ++i) {
                const double st = a.starts[i * a.C + c + 1];
                const double d = fabs(double(fx[i * a.C + c]) - st) / fmax(fabs(st), 1.0);
                gap = (d == d) ? fmax(gap, d) : __builtin_inf();
            }
        }
    }
    red[tid] = gap;
    redb[tid] = bad;
    __syncthreads();
    for (int w = blockDim.x / 2; w > 0; w >>= 1) {
        if (tid < w) {
            red[tid] = fmax(red[tid], red[tid + w]);
            redb[tid] |= redb[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        StreamCheck* k = a.check;
        k->state_gap = red[0];
        k->bad |= redb[0];
        const bool ok = k->bad == 0 && k->cov_gap <= a.tol_cov && red[0] <= a.tol_state;
        k->ok = ok ? 1 : 0;
        if (ok) {
            const int64_t c = a.C - 1;
            for (int i = 0; i < M::N; ++i) static_cast<T*>(a.hx)[i] = fx[i * a.C + c];
            for (int r = 0; r < M::NBLK; ++r) static_cast<T*>(a.hP)[r] = static_cast<const T*>(a.fP)[r * a.C + c];
            a.hstatus[0] = 0;
        }
    }
}
}  // namespace

template <typename T, class M>
void stream_phase(int phase, const StreamArgs& a, hipStream_t stream) {
    constexpr int NCH = M::NP + M::NA;
    auto grid = [](int64_t n) { return dim3(static_cast<unsigned>((n + kBlock - 1) / kBlock)); };
    switch (phase) {
        case 0: stream_init_kernel<T, M><<<grid(a.C), kBlock, 0, stream>>>(a); break;
        case 1: stream_perturb_kernel<T, M><<<grid(4 * a.C), kBlock, 0, stream>>>(a); break;
        case kStreamPhaseScanTiles: {
            const dim3 g(unsigned((a.C + kScanTile - 1) / kScanTile), NCH);
            stream_scan_tiles_kernel<T, M><<<g, kScanTile, 0, stream>>>(a);
            break;
        }
        case kStreamPhaseTop:
            stream_top_kernel<T, M><<<dim3(1, NCH), kScanTile, 0, stream>>>(a);
            break;
        case kStreamPhaseStarts: {
            const dim3 g(unsigned((a.C + kScanTile - 1) / kScanTile), NCH);
            stream_starts_kernel<T, M><<<g, kScanTile, 0, stream>>>(a);
            break;
        }
        case kStreamPhaseLftMaps: {
            const int64_t lanes = a.C * a.np * lft_map_chains<M>(a.sym != 0) * kLftStride;
            KF_CUSTOM_DISPATCH(a.kc, stream_lft_maps_kernel<T, M, CUSTOM><<<grid(lanes), kBlock, 0, stream>>>(a));
            break;
        }
        case kStreamPhaseLftStart: {
            const int64_t bc = a.g > 0 ? a.G : kBlock;
            // LDS variant: G / g threads walk, but the whole block stages the window maps (more
            // loads in flight; the extra threads leave after the staging)
            const unsigned walkers = a.g > 0 ? unsigned((a.G + a.g - 1) / a.g) : unsigned(kBlock);
            const unsigned want = a.start_threads > 0 ? unsigned(a.start_threads) : unsigned(kBlock);
            const unsigned threads = a.g > 0 ? (want > walkers && want <= unsigned(kBlock) ? want : walkers)
                                             : unsigned(kBlock);
            const bool fixed = a.g > 0 && (a.G + a.iters) * a.np <= kStartNu;
            const size_t lds = !(a.g > 0) ? 0
                               : fixed    ? size_t(kStartNu) * 36 * sizeof(double)
                                          : size_t(a.G + a.iters) * a.np * 36 * sizeof(double);
            const dim3 g(unsigned((a.C + bc - 1) / bc), NCH);
            if (fixed) stream_lft_start_kernel<T, M, true, true><<<g, threads, lds, stream>>>(a);
            else if (a.g > 0) stream_lft_start_kernel<T, M, true><<<g, threads, lds, stream>>>(a);
            else stream_lft_start_kernel<T, M, false><<<g, threads, 0, stream>>>(a);
            break;
        }
        case 5: stream_finish_kernel<T, M><<<1, 1024, 0, stream>>>(a); break;
        case kStreamPhaseRecords:
            if constexpr (M::NTRAJ % 2 == 0 && kStreamRecordPairs) {
                // (a caller's trajectory that is not aligned to a pair takes the one-entry kernel)
                if (a.dtab && reinterpret_cast<uintptr_t>(a.traj) % (2 * sizeof(T)) == 0) {
                    stream_records2_kernel<T, M><<<grid(a.S * (M::NTRAJ / 2)), kBlock, 0, stream>>>(a);
                    break;
                }
            }
            stream_records_kernel<T, M><<<grid(a.S * M::NTRAJ), kBlock, 0, stream>>>(a);
            break;
        default: break;
    }
}

hipError_t launch_stream_phase(int model, bool f64, int phase, const StreamArgs& a, hipStream_t stream) {
    if (a.C < 2 || phase < 0 || phase > kStreamPhaseRecords) return hipErrorInvalidValue;
    if (model != 15 && model != 8) return hipErrorInvalidValue;
    KF_MODEL_DISPATCH(model, f64, stream_phase<T, M>(phase, a, stream));
    return hipGetLastError();
}

namespace {
// launch_stream_choose (kf_internal.h): one block; 64 segments of 1024 consecutive flags spread
// evenly over the stream (or every flag of a shorter one), coalesced byte loads, an LDS count
__global__ void __launch_bounds__(1024) stream_choose_kernel(StreamCheck* k, const uint8_t* up, int64_t T,
                                                             int share_den) {
    __shared__ int total;
    const int tid = int(threadIdx.x);
    if (tid == 0) total = 0;
    __syncthreads();
    constexpr int kSeg = 64, kSegLen = 1024;
    int cnt = 0;
    int64_t seen = 0;
    if (T <= int64_t(kSeg) * kSegLen) {
        for (int64_t i = tid; i < T; i += kSegLen) cnt += up[i] != 0;
        seen = T;
    } else {
        for (int j = 0; j < kSeg; ++j) cnt += up[(T - kSegLen) * j / (kSeg - 1) + tid] != 0;
        seen = int64_t(kSeg) * kSegLen;
    }
    atomicAdd(&total, cnt);
    __syncthreads();
    if (tid != 0) return;
    const int ok = k->ok;
    const bool look = int64_t(total) * share_den <= seen;
    k->skip_chain = (ok || look) ? 1 : 0;
    k->skip_gated = (ok || !look) ? 1 : 0;
}
}  // namespace

hipError_t launch_stream_choose(StreamCheck* check, const uint8_t* updated, int64_t T, int share_den,
                                hipStream_t stream) {
    if (!check || !updated || T <= 0 || share_den < 1) return hipErrorInvalidValue;
    stream_choose_kernel<<<1, 1024, 0, stream>>>(check, updated, T, share_den);
    return hipGetLastError();
}

}  // namespace kfmi

// gfx950 kernels for the reference's chain-structured GPS+IMU models (the model layer and the
// layout: kf_ref_model.h): the phases of the time-parallel stream run, the scheduler and the
// schedule search.  The other families have units of their own: kf_ref_lane.hip,
// kf_ref_search.hip, and the 8-lanes-per-filter kf_ref_chain.hip and kf_ref_sweep.hip.
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

// ------------------------------------------------------------------------------------
// Schedule search (kf_search_schedules): the notebook's run_brute_force_kalman_filter
// (KF_SensorFusion.ipynb), one pick per sampling window, scored by position RMSE.  See
// ScheduleArgs (kf_internal.h) for the level layout.
// ------------------------------------------------------------------------------------
// M15 with its (pos, vel, acc) chains only: the same state indices (so a handle's constants are
// read at the same places) and no (att, rate) chain, whose loops in Chains then run no trip.
struct M15Pos : M15 {
    static constexpr int NA = 0;
};

template <bool CUSTOM>
struct ScheduleNode {
    Chains<double, M15Pos, CUSTOM> s;
    double sse;  // running sum over the picks of |position - reference position|^2

    __device__ __forceinline__ void root(const ScheduleArgs& a) {
        s.kc = a.kc;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s.x[M15::pva(c, k)] = a.init[M15::pva(c, k)];
#pragma unroll
            for (int k = 0; k < 6; ++k) s.pva[c][k] = a.init[15 + 6 * c + k];
        }
        sse = 0.0;
    }
    // rows: 3c + k the state of chain c, 9 + 6c + k its packed covariance, 27 the sse
    __device__ __forceinline__ void load(const ScheduleArgs& a, const double* base, uint64_t stride, uint64_t i) {
        s.kc = a.kc;
        const double* p = base + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int k = 0; k < 3; ++k) s.x[M15::pva(c, k)] = p[uint64_t(3 * c + k) * stride];
#pragma unroll
            for (int k = 0; k < 6; ++k) s.pva[c][k] = p[uint64_t(9 + 6 * c + k) * stride];
        }
        sse = p[uint64_t(27) * stride];
    }
    __device__ __forceinline__ void store(double* base, uint64_t stride, uint64_t i) const {
        double* p = base + i;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
#pragma unroll
            for (int k = 0; k < 3; ++k) p[uint64_t(3 * c + k) * stride] = s.x[M15::pva(c, k)];
#pragma unroll
            for (int k = 0; k < 6; ++k) p[uint64_t(9 + 6 * c + k) * stride] = s.pva[c][k];
        }
        p[uint64_t(27) * stride] = sse;
    }
    // The pick of candidate column ci: predict over its time since the previous pick, its update
    // (Chains::event without a gate), then its squared position error.  Returns its time.
    __device__ __forceinline__ double step(const ScheduleArgs& a, uint32_t ci, double t_prev) {
        const double* cd = a.cand + ci;
        const uint64_t C = uint64_t(a.C);
        const double t = cd[0];
        const int type = int(cd[C]);
        double pay[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) pay[i] = cd[uint64_t(2 + i) * C];
        const double dt = t_prev == t_prev ? t - t_prev : 0.0;  // NaN: no previous time yet
        bool ok = true;
        s.template event<false>(type, dt, pay, false, 0.0, ok);
        if (!ok) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
#pragma unroll
                for (int k = 0; k < 3; ++k) s.x[M15::pva(c, k)] = quiet_nan<double>();
#pragma unroll
                for (int k = 0; k < 6; ++k) s.pva[c][k] = quiet_nan<double>();
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double d = s.x[M15::pva(c, 0)] - cd[uint64_t(11 + c) * C];
            sse = fmaT(d, d, sse);
        }
        return t;
    }
};

// lexicographic min of (key, rank) and the sum of cnt over a workgroup of kBlock lanes; the
// result is lane 0's.  The min is exact and order-free, so every run gives the same result.
__device__ __forceinline__ void schedule_block_min(uint64_t& key, uint64_t& rank, uint64_t& cnt) {
    __shared__ uint64_t sk[kBlock], sr[kBlock], sc[kBlock];
    const int tid = int(threadIdx.x);
    sk[tid] = key;
    sr[tid] = rank;
    sc[tid] = cnt;
    __syncthreads();
    for (int h = kBlock / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const uint64_t k2 = sk[tid + h], r2 = sr[tid + h];
            if (k2 < sk[tid] || (k2 == sk[tid] && r2 < sr[tid])) {
                sk[tid] = k2;
                sr[tid] = r2;
            }
            sc[tid] += sc[tid + h];
        }
        __syncthreads();
    }
    key = sk[0];
    rank = sr[0];
    cnt = sc[0];
}

// waves_per_eu(3): the leaf instantiation sits at the 168-VGPR edge of three waves per SIMD
template <bool CUSTOM, bool LEAF>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void ref15_schedule_kernel(
    const ScheduleArgs a) {
    uint64_t bkey = ~uint64_t(0), brank = ~uint64_t(0), cnt = 0;
    const uint64_t stride = uint64_t(gridDim.x) * kBlock;
    const bool narrow = a.n_nodes <= 0xffffffffull;  // 32-bit divisions where the level allows
    for (uint64_t r = uint64_t(blockIdx.x) * kBlock + threadIdx.x; r < a.n_nodes; r += stride) {
        ScheduleNode<CUSTOM> nd;
        double tp;
        uint32_t digit;
        if (a.first) {
            nd.root(a);
            tp = a.prev_time;
            for (int i = 0; i < a.n_fixed; ++i) tp = nd.step(a, uint32_t(ro(a.fixed_idx)[i]), tp);
            digit = uint32_t(r);
        } else {
            uint64_t p;
            if (narrow) p = uint32_t(r) / uint32_t(a.q);
            else p = r / uint64_t(a.q);
            digit = uint32_t(r - p * uint64_t(a.q));
            nd.load(a, a.par, a.n_nodes / uint64_t(a.q), p);
            const uint32_t pd = narrow ? uint32_t(p) % uint32_t(a.q_par) : uint32_t(p % uint64_t(a.q_par));
            tp = a.cand[uint32_t(a.off_par) + pd];
        }
        if (a.q > 0) nd.step(a, uint32_t(a.off) + digit, tp);
        if constexpr (LEAF) {
            const double metric = sqrt(nd.sse / double(a.W));
            if (a.metric_out) a.metric_out[r] = metric;
            if (metric < __builtin_inf()) {  // NaN and +inf never win and are not counted
                ++cnt;
                const uint64_t key = __builtin_bit_cast(uint64_t, metric);  // metric >= 0: its bits order as it does
                if (key < bkey) {  // this lane's ranks ascend: a tie keeps the smaller
                    bkey = key;
                    brank = r;
                }
            }
        } else {
            nd.store(a.child, a.n_nodes, r);
        }
    }
    if constexpr (LEAF) {
        schedule_block_min(bkey, brank, cnt);
        if (threadIdx.x == 0) {
            a.partials[uint64_t(blockIdx.x) * 3 + 0] = bkey;
            a.partials[uint64_t(blockIdx.x) * 3 + 1] = brank;
            a.partials[uint64_t(blockIdx.x) * 3 + 2] = cnt;
        }
    }
}

__global__ __launch_bounds__(kBlock) void schedule_finish_kernel(const uint64_t* partials, int n, uint64_t* host) {
    uint64_t bkey = ~uint64_t(0), brank = ~uint64_t(0), cnt = 0;
    for (int i = int(threadIdx.x); i < n; i += kBlock) {
        const uint64_t k = partials[3 * i], r = partials[3 * i + 1];
        if (k < bkey || (k == bkey && r < brank)) {
            bkey = k;
            brank = r;
        }
        cnt += partials[3 * i + 2];
    }
    schedule_block_min(bkey, brank, cnt);
    if (threadIdx.x == 0) {
        host[0] = bkey;
        host[1] = brank;
        host[2] = cnt;
    }
    __threadfence_system();
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

hipError_t launch_ref15_schedule(const ScheduleArgs& a, bool leaf, hipStream_t stream) {
    if (a.W < 1 || a.n_nodes == 0 || a.q < 0 || a.q > kScheduleMaxQueue || !a.cand || !a.init ||
        (a.n_fixed > 0 && !a.fixed_idx) || (leaf ? !a.partials : !a.child))
        return hipErrorInvalidValue;
    if (a.first ? a.n_nodes != uint64_t(a.q > 0 ? a.q : 1)
                : (a.q < 1 || a.q_par < 1 || !a.par || a.n_nodes % uint64_t(a.q) != 0))
        return hipErrorInvalidValue;
    if (!leaf && a.n_nodes > kScheduleMaxNodes) return hipErrorInvalidValue;
    const dim3 grid(schedule_grid(a.n_nodes));
    KF_CUSTOM_DISPATCH(a.kc, KF_BOOL_DISPATCH(leaf, LEAF, ref15_schedule_kernel<CUSTOM, LEAF><<<grid, kBlock, 0, stream>>>(a)));
    return hipGetLastError();
}

hipError_t launch_schedule_finish(const uint64_t* partials, int n, uint64_t* host, hipStream_t stream) {
    if (n < 1 || n > int(kScheduleGrid) || !partials || !host) return hipErrorInvalidValue;
    schedule_finish_kernel<<<1, kBlock, 0, stream>>>(partials, n, host);
    return hipGetLastError();
}

}  // namespace kfmi

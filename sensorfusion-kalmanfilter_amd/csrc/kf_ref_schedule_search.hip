// The schedule search of the 15-state model (kf_ref_model.h), kf_search_schedules: one pick per
// sampling window, by levels over a shared prefix, scored by position RMSE
// (launch_ref15_schedule) and reduced to the best schedule (launch_schedule_finish).
#include "kf_ref_model.h"

namespace kfmi {
namespace {

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

// The one-lane-per-filter kernels of the reference models (the model layer: kf_ref_model.h):
// ref_events_kernel, its LDS-staged variant and the reset.  They serve kf_run_events and
// kf_run_events_gates (launch_ref_events, which forwards the chain and look-ahead variants to
// kf_ref_chain.hip) and kf_reset (launch_ref_reset).
#include "kf_ref_model.h"

namespace kfmi {
namespace {

// ------------------------------------------------------------------------------------
// Per-filter event streams (kf_run_events).
// ------------------------------------------------------------------------------------
template <typename T, class M, bool CUSTOM, bool GATES = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void ref_events_kernel(const RefArgs a) {
    const int64_t f = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (f >= a.B) return;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(a.B) * uint32_t(sizeof(T));
    const uint32_t rb8 = uint32_t(a.B) * 8u;
    const uint32_t off8 = uint32_t(f) * 8u;
    Chains<T, M, CUSTOM> s;
    s.kc = a.kc;
    s.load(a.x, a.P, rb, off);
    int32_t st = a.status[f];
    FilterGate<T> fg{false, T(0)};
    if constexpr (GATES) fg = gate_of<T>(a.thresholds, f);
    const uint32_t rb_tr = a.traj ? rb : 0u, rb_ld = a.logdet ? rb : 0u, rb_cv = a.cov ? rb : 0u;
    struct In {
        int type;
        double dt;
        T pay[9];
    };
    auto load = [&](int t, In& in) {
        in.type = int(ldb<uint8_t>(a.etype, t, uint32_t(a.B), uint32_t(f)));
        in.dt = ldb<double>(a.dt, t, rb8, off8);
#pragma unroll
        for (int i = 0; i < 9; ++i) in.pay[i] = ldb<T>(a.payload, int64_t(t) * 9 + i, rb, off);
    };
    auto step = [&](int t, const In& in) {
        bool applied = false;
        if (in.type != 255) {
            bool ok = true;
            applied = s.template event<false>(in.type, T(in.dt), in.pay, GATES ? fg.on : a.gate != 0,
                                              GATES ? fg.thr : T(a.threshold), ok);
            if (!ok) {
                st = kNotSpd;
                s.fill_nan();
            }
        }
#pragma unroll
        for (int i = 0; i < M::NTRAJ; ++i) stb(a.traj, int64_t(t) * M::NTRAJ + i, rb_tr, off, s.x[i]);
        if (a.cov) s.store_cov(a.cov, int64_t(t) * M::NBLK, rb_cv, off);
        if (a.logdet) {
            const T ld = s.logdet();
            st = (ld == ld) ? st : kNotSpd;
            stb(a.logdet, t, rb_ld, off, ld);
        }
        if (a.updated) a.updated[int64_t(t) * a.B + f] = applied ? 1 : 0;
    };
    // no prefetch: at 3 waves/SIMD this kernel is instruction-bound, and a second input buffer
    // (A/B-measured: 8.93 vs 9.00 ms at B = 2^20, T = 256) costs a wave of occupancy
    for (int t = 0; t < a.T; ++t) {
        In in;
        load(t, in);
        step(t, in);
    }
    s.store(a.x, a.P, rb, off);
    a.status[f] = st;
}

// ------------------------------------------------------------------------------------
// ref_events_kernel with its inputs staged through LDS by the DMA engine (buffer_load ... lds):
// event t+1's payload, dt and type travel HBM -> LDS while event t computes, without VGPRs
// (a register prefetch of the same inputs costs this fp64 kernel its third wave per SIMD).
// Each wave owns one LDS image of an event's inputs:
//   [0, 9*64*W)              payload rows 0..8, 64 filters each (row-major, lane-linear)
//   [DT_OFF, DT_OFF + 512)   dt, 64 doubles
//   [ET_OFF, ET_OFF + 64)    event type, 64 bytes
// Every DMA instruction moves 64 lanes x 16 B of ONE input (a wave-uniform row-span descriptor,
// the lane's chunk in voffset; the range check drops what lies beyond the span).  Order per
// event: wait for the image (counted vmcnt: only the previous event's NST stores are younger),
// read it into registers, drain those reads (lgkmcnt), issue the next event's DMA into the same
// image, compute, store.  The per-event store count NST is fixed (absent records go to
// zero-length descriptors) so the wait can be counted.  Requires B % 16 == 0 (no 16-B chunk
// straddles B) and 9 * B * W < 2^32; the host falls back to ref_events_kernel otherwise.
// ------------------------------------------------------------------------------------

// payload element i of this lane, read from the wave's LDS image where the update uses it
template <typename T>
struct LdsPayload {
    const T* img;  // image base + lane
    __device__ __forceinline__ T operator[](int i) const { return img[i * 64]; }
};

template <typename T, class M, bool COV, bool CUSTOM, bool GATES = false>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(3))) void ref_events_lds_kernel(
    const RefArgs a) {
    constexpr int W = int(sizeof(T));
    constexpr int PAY = 9 * 64 * W;
    constexpr int NIP = (PAY + 1023) / 1024;    // payload DMA instructions
    constexpr int LPR = 4 * W;                  // lanes per 64-filter row (16 B each)
    constexpr int DT_OFF = NIP * 1024, ET_OFF = DT_OFF + 1024, IMG = ET_OFF + 64;
    constexpr int NDMA = NIP + 2;
    constexpr int NST = M::NTRAJ + 2 + (COV ? M::NBLK : 0);  // traj, logdet, updated (+ cov)
    static_assert(NST + NDMA <= 63, "vmcnt range");
    __shared__ __attribute__((aligned(16))) unsigned char lds[(kBlock / 64) * 2 * IMG];
    const int lane = int(threadIdx.x & 63);
    const int wave = wave_uniform(int(threadIdx.x >> 6));
    const int64_t f0 = int64_t(blockIdx.x) * kBlock + int64_t(wave) * 64;
    if (f0 >= a.B) return;  // whole wave; partial waves keep their dead lanes for the DMA
    const int64_t f = f0 + lane;
    unsigned char* const img0 = lds + wave * 2 * IMG;
    const uint32_t off = uint32_t(f) * uint32_t(W);  // dead lanes: beyond every row
    const uint32_t rb = uint32_t(a.B) * uint32_t(W);
    Chains<T, M, CUSTOM> s;
    s.kc = a.kc;
    s.load(a.x, a.P, rb, off);
    int32_t st = f < a.B ? a.status[f] : 0;
    FilterGate<T> fg{false, T(0)};  // loaded with the state, ahead of the drain below
    if constexpr (GATES) fg = gate_of<T>(a.thresholds, f < a.B ? f : a.B - 1);
    const uint32_t rb_tr = a.traj ? rb : 0u, rb_ld = a.logdet ? rb : 0u, rb_cv = a.cov ? rb : 0u;
    const uint32_t rb_up = a.updated ? uint32_t(a.B) : 0u;
    // drain the state loads once: left pending into the loop, the waitcnt pass puts a wait for
    // them at each first use in every iteration, and those waits would drain the DMA prefetch
    waitcnt<vmcnt_imm(0)>();
    // payload DMA instruction k moves rows 16/W*k + lane / LPR, 16-B chunk lane % LPR of each;
    // the row step k * (16/W) * rb goes into soffset
    const uint32_t voff_pay = uint32_t(lane / LPR) * rb + uint32_t(lane % LPR) * 16u;
    auto issue = [&](int t, unsigned char* img) {
        const char* pb = reinterpret_cast<const char*>(a.payload) + int64_t(t) * 9 * int64_t(rb) + f0 * W;
        const __amdgpu_buffer_rsrc_t rp = bytes_rsrc(pb, 9u * rb - uint32_t(f0) * W);
#pragma unroll
        for (int k = 0; k < NIP; ++k)
            if (k + 1 < NIP || k * 1024 + lane * 16 < PAY)
                lds_dma16(rp, img + k * 1024, voff_pay, k * (16 / W) * int(rb));
        const char* db = reinterpret_cast<const char*>(a.dt) + int64_t(t) * int64_t(a.B) * 8 + f0 * 8;
        if (lane < 32) lds_dma16(bytes_rsrc(db, uint32_t(a.B - f0) * 8u), img + DT_OFF, uint32_t(lane) * 16u, 0);
        const char* eb = reinterpret_cast<const char*>(a.etype) + int64_t(t) * int64_t(a.B) + f0;
        if (lane < 4) lds_dma16(bytes_rsrc(eb, uint32_t(a.B - f0)), img + ET_OFF, uint32_t(lane) * 16u, 0);
    };
    issue(0, img0);
    // the in-loop count assumes a previous event's NST stores are younger than this image's
    // DMA; event 0 has none, so its image is waited for here
    waitcnt<vmcnt_imm(0)>();
    for (int t = 0; t < a.T; ++t) {
        unsigned char* const img = img0 + (t & 1) * IMG;
        // the other image was last read by event t - 1, whose reads have completed
        if (t + 1 < a.T) {
            issue(t + 1, img0 + ((t + 1) & 1) * IMG);
            // event t's image: its DMA is older than event t-1's NST stores and this NDMA
            waitcnt<vmcnt_imm(NST + NDMA)>();
        } else {
            waitcnt<vmcnt_imm(NST)>();
        }
        const int type = img[ET_OFF + lane];
        const T dt = T(reinterpret_cast<const double*>(img + DT_OFF)[lane]);
        const LdsPayload<T> pay{reinterpret_cast<const T*>(img) + lane};
        bool applied = false;
        if (type != 255) {
            bool ok = true;
            applied = s.template event<false>(type, dt, pay, GATES ? fg.on : a.gate != 0, GATES ? fg.thr : T(a.threshold),
                                              ok);
            if (!ok) {
                st = kNotSpd;
                s.fill_nan();
            }
        }
#pragma unroll
        for (int i = 0; i < M::NTRAJ; ++i) stb(a.traj, int64_t(t) * M::NTRAJ + i, rb_tr, off, s.x[i]);
        if constexpr (COV) s.store_cov(a.cov, int64_t(t) * M::NBLK, rb_cv, off);
        const T ld = a.logdet ? s.logdet() : T(0);
        st = (ld == ld) ? st : kNotSpd;
        stb(a.logdet, t, rb_ld, off, ld);
        stb_u8(a.updated, t, rb_up, uint32_t(f), applied ? uint8_t(1) : uint8_t(0));
    }
    s.store(a.x, a.P, rb, off);
    if (f < a.B) a.status[f] = st;
}

template <typename T, class M, bool CUSTOM>
__global__ __launch_bounds__(kBlock) void ref_reset_kernel(const RefArgs a) {
    const int64_t f = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (f >= a.B) return;
    const uint32_t off = uint32_t(f) * uint32_t(sizeof(T));
    const uint32_t rb = uint32_t(a.B) * uint32_t(sizeof(T));
    Chains<T, M, CUSTOM> s;
    s.kc = a.kc;
#pragma unroll
    for (int i = 0; i < M::N; ++i) s.x[i] = a.x0 ? ldb<T>(a.x0, i, rb, off) : T(0);
    s.reset_cov();
    s.store(a.x, a.P, rb, off);
    a.status[f] = 0;
}
}  // namespace

namespace {
// kf_run_events' one-lane-per-filter kernels; GATES (a.thresholds, kf_run_events_gates): the same
// kernels with per-filter gates
template <typename T, class M, bool CUSTOM, bool GATES>
void ref_events_t(const RefArgs& a, hipStream_t stream, int variant) {
    const dim3 grid(static_cast<unsigned>((a.B + kBlock - 1) / kBlock));
    if (variant == kEventsLds)
        KF_BOOL_DISPATCH(a.cov, COV, ref_events_lds_kernel<T, M, COV, CUSTOM, GATES><<<grid, kBlock, 0, stream>>>(a));
    else
        ref_events_kernel<T, M, CUSTOM, GATES><<<grid, kBlock, 0, stream>>>(a);
}
}  // namespace

hipError_t launch_ref_events(int model, bool f64, const RefArgs& a, hipStream_t stream, int variant) {
    if (model != 15 && model != 8) return hipErrorInvalidValue;
    if (a.thresholds && (variant == kEventsGated || a.s_len != 0)) return hipErrorInvalidValue;
    if (variant == kEventsChain || variant == kEventsGated) return launch_ref_events_chain(model, f64, a, stream, variant);
    KF_REF_DISPATCH(model, f64, a.kc,
                    KF_BOOL_DISPATCH(a.thresholds, GATES, ref_events_t<T, M, CUSTOM, GATES>(a, stream, variant)));
    return hipGetLastError();
}

hipError_t launch_ref_reset(int model, bool f64, const RefArgs& a, hipStream_t stream) {
    const dim3 grid(static_cast<unsigned>((a.B + kBlock - 1) / kBlock));
    if (model != 15 && model != 8) return hipErrorInvalidValue;
    KF_REF_DISPATCH(model, f64, a.kc, ref_reset_kernel<T, M, CUSTOM><<<grid, kBlock, 0, stream>>>(a));
    return hipGetLastError();
}

}  // namespace kfmi

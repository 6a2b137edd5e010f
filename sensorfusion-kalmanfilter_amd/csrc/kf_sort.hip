// The device radix sort of (key, value) pairs that the scheduler's launcher orders its waves with
// (sort_pairs_desc_u32, declared in kf_internal.h): a thin wrapper over hipCUB, in a unit of its
// own so that the reference units compile no library templates and the ingest unit only its own.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <hipcub/hipcub.hpp>

#include "kf_internal.h"

namespace kfmi {
hipError_t sort_pairs_desc_u32(void* tmp, size_t* tmp_bytes, const uint32_t* keys_in, uint32_t* keys_out,
                               const uint32_t* vals_in, uint32_t* vals_out, int n, int bits, hipStream_t stream) {
    return hipcub::DeviceRadixSort::SortPairsDescending(tmp, *tmp_bytes, keys_in, keys_out, vals_in, vals_out, n, 0,
                                                        bits, stream);
}
}  // namespace kfmi

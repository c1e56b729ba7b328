// Test infrastructure (not the product): fills every CU's LDS with a pattern, so that a trace kernel launched afterwards finds
// that pattern -- not whatever the previous kernel happened to leave -- in the ring slots it has not written yet.  A round of
// fewer than 64 pairs reads such slots (rl_scan_wave: the lanes beyond the round are pointed at record 0 before anything is
// loaded through them); with all ones in them a kernel that loaded through a stale entry from global memory would fault.
// lds_peek is the positive control: a kernel of the same shape that only READS its LDS and counts the words that still hold the
// pattern, so that a test can tell whether what lds_poison wrote is what the next kernel finds (tests/test_gpu_dirty_state.py).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

__global__ __launch_bounds__(1024) void poison_kernel(uint32_t pattern, uint32_t n_words, unsigned long long* sink) {
    extern __shared__ uint32_t lds[];
    for (uint32_t i = threadIdx.x; i < n_words; i += 1024) lds[i] = pattern;
    __syncthreads();
    // (read one word back so that the stores are not dead code)
    if (threadIdx.x == 0 && lds[(blockIdx.x * 977u) % n_words] != pattern) atomicAdd(sink, 1ull);
}

// Never writes its LDS: every word is read as the previous kernel on this CU left it, and the workgroup's count of words equal to
// `pattern` is added to found[blockIdx.x] in global memory (one atomic per wave).
__global__ __launch_bounds__(1024) void peek_kernel(uint32_t pattern, uint32_t n_words, uint32_t* found) {
    extern __shared__ uint32_t lds[];
    const volatile uint32_t* words = lds;
    uint32_t mine = 0;
    for (uint32_t i = threadIdx.x; i < n_words; i += 1024) mine += words[i] == pattern ? 1u : 0u;
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63u) == 0 && mine != 0) atomicAdd(&found[blockIdx.x], mine);
}

static const size_t kLdsBytes = 160 * 1024;

// Returns 0 on success.  `blocks` workgroups of 1024 threads with the CU's whole 160 KB each: one per CU at a time, so a grid of a
// few times the CU count reaches every CU.
extern "C" int lds_poison(int device, uint32_t pattern, uint32_t blocks) {
    if (hipSetDevice(device) != hipSuccess) return 1;
    const size_t bytes = kLdsBytes;
    if (hipFuncSetAttribute((const void*)poison_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return 2;
    unsigned long long* sink = nullptr;
    if (hipMalloc((void**)&sink, sizeof *sink) != hipSuccess) return 3;
    (void)hipMemset(sink, 0, sizeof *sink);
    hipLaunchKernelGGL(poison_kernel, dim3(blocks), dim3(1024), bytes, 0, pattern, (uint32_t)(bytes / 4), sink);
    int rc = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : 4;
    unsigned long long bad = 0;
    if (rc == 0 && hipMemcpy(&bad, sink, sizeof bad, hipMemcpyDeviceToHost) != hipSuccess) rc = 5;
    (void)hipFree(sink);
    return rc != 0 ? rc : (bad != 0 ? 6 : 0);
}

// The same grid shape and 160 KB of dynamic LDS as lds_poison.  Returns 0 on success and then
//   *groups_found:   the workgroups that read `pattern` in at least one word,
//   *words_found:    the words equal to `pattern`, summed over all workgroups,
//   *words_per_group: the words one workgroup read (160 KB / 4),
//   per_group:       NULL, or room for `blocks` counts: the words equal to `pattern` each workgroup read.
extern "C" int lds_peek(int device, uint32_t pattern, uint32_t blocks, uint64_t* groups_found, uint64_t* words_found,
                        uint64_t* words_per_group, uint32_t* per_group) {
    if (hipSetDevice(device) != hipSuccess) return 1;
    if (blocks == 0 || !groups_found || !words_found || !words_per_group) return 7;
    const size_t bytes = kLdsBytes;
    if (hipFuncSetAttribute((const void*)peek_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return 2;
    uint32_t* found = nullptr;
    if (hipMalloc((void**)&found, blocks * sizeof *found) != hipSuccess) return 3;
    (void)hipMemset(found, 0, blocks * sizeof *found);
    hipLaunchKernelGGL(peek_kernel, dim3(blocks), dim3(1024), bytes, 0, pattern, (uint32_t)(bytes / 4), found);
    int rc = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess ? 0 : 4;
    std::vector<uint32_t> host(blocks, 0u);
    if (rc == 0 && hipMemcpy(host.data(), found, blocks * sizeof *found, hipMemcpyDeviceToHost) != hipSuccess) rc = 5;
    (void)hipFree(found);
    if (rc != 0) return rc;
    *groups_found = *words_found = 0;
    *words_per_group = bytes / 4;
    for (uint32_t b = 0; b < blocks; ++b) {
        *groups_found += host[b] != 0 ? 1u : 0u;
        *words_found += host[b];
        if (per_group) per_group[b] = host[b];
    }
    return 0;
}

// The device's compute units as the runtime reports them (hipDeviceProp_t::multiProcessorCount), or -1.
extern "C" int lds_cu_count(int device) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return -1;
    return prop.multiProcessorCount;
}

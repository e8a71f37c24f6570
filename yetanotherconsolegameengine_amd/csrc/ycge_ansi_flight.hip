// ycge_ansi_flight.hip - the delivery of an ANSI stream with frames in flight (ycge_render_frame_async_ansi; host side: ycge_ansi.cpp; the
// contract: include/ycge.h).
//
// The synchronous calls read the stream's length on the host and copy exactly that many bytes, which takes a synchronisation inside the
// call.  k_ansi_deliver runs behind a stream's scan and write kernels on the same HIP stream instead: it reads the length (a delta: and the
// three counters) from the words k_scan wrote, copies exactly that many bytes of the device stream into the caller's page-locked buffer
// through its device alias, and fills the caller's result record.  The host learns nothing during the call.
//   - a fixed grid of 256-lane workgroups strides over 16-byte units: consecutive lanes store consecutive units, one 16-byte vector store
//     each (both buffers are 16-byte aligned at their base);
//   - the tail of fewer than 16 bytes is stored bytewise from bytewise loads: no load passes src + length, no store dst + length;
//   - length > capacity (the host's capacity check makes that a kernel bug elsewhere): nothing is copied, status = 1 in the record and
//     one sticky word of the library's page-locked memory is set, which join_async reports.
// No LDS, no atomics, no scratch.  Its own translation unit: the code objects of the stream kernels stay what they were.
#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kDeliverBlock = 256;

// ycge_ansi_async_result (include/ycge.h), 32 bytes
struct DeliverRecord {
    unsigned long long length;
    uint32_t info[4];            // {keyframe returned, changed, emitted, run starts}
    uint32_t status, reserved;
};
static_assert(sizeof(DeliverRecord) == 32, "ycge_ansi_async_result is 32 bytes");

// res: {length, changed, emitted, run starts} as k_scan<true> wrote them (full: k_scan<false> wrote the length alone - the counters are not read)
__global__ __launch_bounds__(kDeliverBlock) void k_ansi_deliver(const uint8_t *__restrict__ src, const unsigned long long *__restrict__ res,
                                                                 unsigned long long capacity, int full, uint8_t *__restrict__ dst,
                                                                 DeliverRecord *__restrict__ rec, uint32_t *__restrict__ sticky)
{
    const unsigned long long len = res[0];
    const bool over = len > capacity;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        rec->length = len;
        rec->info[0] = full ? 1u : 0u;
        for (int k = 1; k < 4; k++) rec->info[k] = full ? 0u : (uint32_t)res[k];
        rec->status = over ? 1u : 0u;
        rec->reserved = 0u;
        if (over) *sticky = 1u;
    }
    if (over) return;
    const size_t units = (size_t)(len >> 4);
    const uint4 *__restrict__ s = reinterpret_cast<const uint4 *>(src);
    uint4 *__restrict__ d = reinterpret_cast<uint4 *>(dst);
    const size_t stride = (size_t)gridDim.x * kDeliverBlock;
    for (size_t u = (size_t)blockIdx.x * kDeliverBlock + threadIdx.x; u < units; u += stride) d[u] = s[u];
    const uint32_t tail = (uint32_t)(len & 15ull);
    if (blockIdx.x == 0 && threadIdx.x < tail) dst[(units << 4) + threadIdx.x] = src[(units << 4) + threadIdx.x];
}

} // namespace

// the delivery of the stream at src whose result words are res, behind whatever wrote them on `stream`: dst (capacity bytes) and record
// (a ycge_ansi_async_result) are device aliases of page-locked host memory, 16- and 8-byte aligned; sticky: one such word of the library's.
// groups: workgroups of 256 lanes (at least 1).  One launch.
extern "C" int ycge_launch_ansi_deliver(const uint8_t *src, const unsigned long long *res, unsigned long long capacity, int full, uint8_t *dst, void *record,
                                        uint32_t *sticky, int groups, hipStream_t stream)
{
    if (!src || !res || !dst || !record || !sticky || ((uintptr_t)src & 15u) || ((uintptr_t)dst & 15u) || ((uintptr_t)record & 7u)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(k_ansi_deliver, dim3((unsigned)(groups > 0 ? groups : 1)), dim3(kDeliverBlock), 0, stream, src, res, capacity, full, dst,
                       static_cast<DeliverRecord *>(record), sticky);
    return (int)hipGetLastError();
}

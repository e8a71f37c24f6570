// ycge_sixel_host.h - the sixel streams in plain C++ (ycge_sixel_host.cpp): the bound, the header, the full stream and the delta stream of
// register planes.  No HIP and no context type: the file compiles on its own, and a stand-alone program can hold it to the contract under
// the host sanitizers (tests/sixel_host_main.cpp).  The contract: include/ycge.h at ycge_render_frame_sixel and ycge_render_frame_sixel_delta.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

namespace ycge_sixel_host {

// 3200 + ceil(H / 6) * min(216, 6 W) * (W + 5); false where W or H is not positive or the bound does not fit 32 bits (the kernels' offsets)
bool stream_bound(int64_t W, int64_t H, unsigned long long &bound);

// parts 1 to 5 of the full stream; delta: the delta stream's parts 1 to 4 - no ESC[2J, and the introducer ESC P 0;1 q (P2 = 1: a zero bit
// leaves its pixel as it is)
std::string stream_header(int32_t W, int32_t H, int32_t vx, int32_t vy, bool clear, bool delta = false);

// ycge_sixel_encode_host and ycge_sixel_encode_delta_host: status codes of include/ycge.h
int encode(const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, int32_t clear, uint8_t *out, size_t capacity, size_t *out_len);
int encode_delta(const uint8_t *prev, const uint8_t *index, int32_t W, int32_t H, int32_t vx, int32_t vy, uint8_t *out, size_t capacity, size_t *out_len,
                 uint32_t *out_info);

} // namespace ycge_sixel_host

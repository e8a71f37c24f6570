// sixel_host_main.cpp - a stand-alone program over the plain C++ sixel encoders (csrc/ycge_sixel_host.cpp), for a build under the host
// sanitizers (tests/test_sixel_delta_cpu.py builds it with -fsanitize=address,undefined and runs it: no library, no device, nothing loaded
// into another process).
//
//   sixel_host_main <jobs> <streams>
// <jobs>: records of int32 {W, H, vx, vy, clear, delta}, then W * H bytes cur, then for delta != 0 W * H bytes prev.
// <streams>: per job int32 status, uint64 length, uint32 info[4], then the stream's bytes - written into a buffer of exactly the bound, so a
// byte past it is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../yetanotherconsolegameengine_amd/csrc/ycge_sixel_host.cpp"

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <jobs> <streams>\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t head[6];
    int jobs = 0;
    while (std::fread(head, sizeof head, 1, in) == 1) {
        const int32_t W = head[0], H = head[1];
        const size_t n = (size_t)W * (size_t)H;
        std::vector<uint8_t> cur(n), prev(head[5] ? n : 0);
        if (std::fread(cur.data(), 1, n, in) != n || (head[5] && std::fread(prev.data(), 1, n, in) != n)) { std::fprintf(stderr, "short job %d\n", jobs); return 2; }
        unsigned long long bound = 0;
        if (!ycge_sixel_host::stream_bound(W, H, bound)) { std::fprintf(stderr, "no bound for job %d\n", jobs); return 2; }
        std::vector<uint8_t> stream((size_t)bound);
        size_t len = 0;
        uint32_t info[4] = {0, 0, 0, 0};
        const int32_t rc = head[5] ? ycge_sixel_host::encode_delta(prev.data(), cur.data(), W, H, head[2], head[3], stream.data(), stream.size(), &len, info)
                                   : ycge_sixel_host::encode(cur.data(), W, H, head[2], head[3], head[4], stream.data(), stream.size(), &len);
        const uint64_t len64 = len;
        std::fwrite(&rc, sizeof rc, 1, out);
        std::fwrite(&len64, sizeof len64, 1, out);
        std::fwrite(info, sizeof info, 1, out);
        std::fwrite(stream.data(), 1, len, out);
        jobs++;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("%d jobs\n", jobs);
    return 0;
}

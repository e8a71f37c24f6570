// sixel_palette_host_main.cpp - a stand-alone program over the plain C++ adaptive palette (csrc/ycge_sixel_host.cpp), for a build under the
// host sanitizers (tests/test_sixel_palette_cpu.py builds it with -fsanitize=address,undefined and runs it: no library, no device, nothing
// loaded into another process).
//
//   sixel_palette_host_main <jobs> <results>
// <jobs>: records of int32 {W, H, vx, vy, clear, hold}, then W * H * 4 bytes RGBA.  hold != 0: the picture is mapped through the palette of
// the job before (palette_map alone), as a context's kept palette would be; else through its own (palette()).
// <results>: per job int32 status, int32 n, uint64 length, 1024 bytes palette, 768 bytes percentages, W * H registers, the stream's bytes -
// every output in a buffer of exactly its size, so a byte past one is the sanitizer's to report.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "../yetanotherconsolegameengine_amd/csrc/ycge_sixel_host.cpp"

int main(int argc, char **argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: %s <jobs> <results>\n", argv[0]); return 2; }
    std::FILE *in = std::fopen(argv[1], "rb"), *out = std::fopen(argv[2], "wb");
    if (!in || !out) { std::fprintf(stderr, "cannot open the files\n"); return 2; }
    int32_t head[6];
    int jobs = 0;
    std::unique_ptr<ycge_sixel_host::KeptPalette> kept(new ycge_sixel_host::KeptPalette());
    bool have = false;
    while (std::fread(head, sizeof head, 1, in) == 1) {
        const int32_t W = head[0], H = head[1];
        const size_t n = (size_t)W * (size_t)H;
        std::vector<uint8_t> rgba(4 * n), index(n), palette(1024), pct(768);
        if (std::fread(rgba.data(), 1, 4 * n, in) != 4 * n) { std::fprintf(stderr, "short job %d\n", jobs); return 2; }
        int32_t count = 0, rc = 0;
        if (head[5] && have) {
            ycge_sixel_host::palette_map(rgba.data(), n, *kept, index.data());
        } else {
            rc = ycge_sixel_host::palette(rgba.data(), W, H, index.data(), palette.data(), pct.data(), &count);
            ycge_sixel_host::palette_build(rgba.data(), n, *kept);
            have = true;
        }
        count = kept->count;
        std::copy(kept->rgba, kept->rgba + 1024, palette.begin());
        std::copy(kept->pct, kept->pct + 768, pct.begin());
        unsigned long long bound = 0;
        if (!ycge_sixel_host::palette_stream_bound(W, H, bound)) { std::fprintf(stderr, "no bound for job %d\n", jobs); return 2; }
        std::vector<uint8_t> stream((size_t)bound);
        size_t len = 0;
        if (rc == 0) rc = ycge_sixel_host::encode_palette(index.data(), pct.data(), count, W, H, head[2], head[3], head[4], stream.data(), stream.size(), &len);
        const uint64_t len64 = len;
        std::fwrite(&rc, sizeof rc, 1, out);
        std::fwrite(&count, sizeof count, 1, out);
        std::fwrite(&len64, sizeof len64, 1, out);
        std::fwrite(palette.data(), 1, palette.size(), out);
        std::fwrite(pct.data(), 1, pct.size(), out);
        std::fwrite(index.data(), 1, n, out);
        std::fwrite(stream.data(), 1, len, out);
        jobs++;
    }
    std::fclose(in);
    if (std::fclose(out) != 0) return 2;
    std::printf("%d jobs\n", jobs);
    return 0;
}

// prog_fuzz_main.cpp -- mutation fuzzer for progressive decoding on the host: the product's parser (SOF2, the scan
// rules, the restart walk), the scan bodies of jg_prog_core.h driven by the host twin, and the hand-over's pack with its
// way back. Built with -fsanitize=address,undefined by tests/test_progressive_fuzz_host.py: an access outside a buffer,
// a misaligned read or an overflow outside -fwrapv's reach aborts the run. Corrupt streams are exercised here only; the
// kernels compile the same jg_prog_core.h.
//
//   prog_fuzz_main <iterations> <seed> file.jpg [file.jpg ...]
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

struct ProgTwinInfo {
    int num_comp, num_scans, num_levels, color_space;
    int size_x[4], size_y[4], blocks_x[4], blocks_y[4], vis_x[4], vis_y[4];
    int scan_level[64], scan_segments[64];
};
extern "C" int prog_twin_run(const uint8_t* data, size_t size, int progressive, int shard_world, ProgTwinInfo* info, int16_t* const* coef, int16_t* const* back);

static uint64_t g_state = 1;
static uint32_t rnd()
{
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return static_cast<uint32_t>(g_state >> 11);
}

int main(int argc, char** argv)
{
    if (argc < 4) return 2;
    const int iterations = std::atoi(argv[1]);
    g_state              = std::strtoull(argv[2], nullptr, 10) * 2654435761u + 88172645463325252ull;
    std::vector<std::vector<uint8_t>> files;
    for (int i = 3; i < argc; ++i) {
        FILE* f = std::fopen(argv[i], "rb");
        if (!f) return 2;
        std::fseek(f, 0, SEEK_END);
        const long n = std::ftell(f);
        std::fseek(f, 0, SEEK_SET);
        std::vector<uint8_t> d(static_cast<size_t>(n));
        if (std::fread(d.data(), 1, d.size(), f) != d.size()) return 2;
        std::fclose(f);
        files.push_back(d);
    }
    int ok = 0, rejected = 0;
    for (int it = 0; it < iterations; ++it) {
        std::vector<uint8_t> d = files[rnd() % files.size()];
        const int kind         = rnd() % 5;
        const int edits        = 1 + rnd() % 8;
        // everything up to the first scan header is where the structural damage goes; kind 2 damages what lies behind it
        // (the later scans' headers and tables included); kind 4 only entropy-coded bytes, and writes no FF there, so that
        // the file keeps its structure and the scan bodies meet the damage
        size_t hdr = d.size();
        for (size_t i = 0; i + 1 < d.size(); ++i)
            if (d[i] == 0xFF && d[i + 1] == 0xDA) { hdr = i + 16 < d.size() ? i + 16 : d.size(); break; }
        std::vector<size_t> coded;
        for (size_t i = 2; kind == 4 && i + 4 <= d.size() && d[i] == 0xFF;) {
            const uint8_t m = d[i + 1];
            if (m == 0xD9) break;
            i += 2 + (static_cast<size_t>(d[i + 2]) << 8 | d[i + 3]);
            if (m != 0xDA) continue;
            for (; i + 1 < d.size() && !(d[i] == 0xFF && d[i + 1] != 0 && !(d[i + 1] >= 0xD0 && d[i + 1] <= 0xD7)); ++i)
                if (d[i] != 0xFF && d[i - 1] != 0xFF) coded.push_back(i);
        }
        for (int e = 0; e < edits; ++e) {
            if (kind == 4) {
                if (coded.empty()) break;
                const size_t pos = coded[rnd() % coded.size()];
                const uint8_t v  = static_cast<uint8_t>(rnd() % 3 == 0 ? 0 : rnd());
                d[pos]           = v == 0xFF ? 0xFE : v;
                continue;
            }
            const size_t pos = kind == 0 ? rnd() % hdr : kind == 1 ? rnd() % d.size() : hdr + rnd() % (d.size() - hdr + 1);
            if (pos >= d.size()) continue;
            switch (rnd() % 4) {
            case 0: d[pos] = static_cast<uint8_t>(rnd()); break;
            case 1: d[pos] ^= static_cast<uint8_t>(1u << (rnd() % 8)); break;
            case 2: d[pos] = 0xFF; break;
            default: d[pos] = 0; break;
            }
        }
        if (kind == 3 && d.size() > 64) d.resize(d.size() - rnd() % (d.size() / 2)); // truncation
        ProgTwinInfo info;
        if (prog_twin_run(d.data(), d.size(), 1, 1, &info, nullptr, nullptr) != 0 || info.num_scans == 0) {
            ++rejected;
            continue;
        }
        size_t blocks = 0;
        for (int c = 0; c < info.num_comp; ++c) blocks += static_cast<size_t>(info.blocks_x[c]) * info.blocks_y[c];
        if (blocks > (size_t{1} << 20)) continue; // absurd geometry claims: skip the allocation
        std::vector<std::vector<int16_t>> coef(4), back(4);
        int16_t *cp[4] = {}, *bp[4] = {};
        for (int c = 0; c < info.num_comp; ++c) {
            coef[c].resize(static_cast<size_t>(info.blocks_x[c]) * info.blocks_y[c] * 64);
            back[c].resize(static_cast<size_t>(info.vis_x[c]) * info.vis_y[c] * 64);
            cp[c] = coef[c].data(), bp[c] = back[c].data();
        }
        if (prog_twin_run(d.data(), d.size(), 1, 1, &info, cp, bp) != 0) return 3; // the same bytes parsed a moment ago
        for (int c = 0; c < info.num_comp; ++c) // the way back returns what was packed, whatever the bits decoded to
            for (int by = 0; by < info.vis_y[c]; ++by)
                for (int bx = 0; bx < info.vis_x[c]; ++bx)
                    for (int k = 0; k < 64; ++k)
                        if (back[c][(static_cast<size_t>(by) * info.vis_x[c] + bx) * 64 + k] != coef[c][(static_cast<size_t>(by) * info.blocks_x[c] + bx) * 64 + k]) return 4;
        ++ok;
    }
    std::printf("fuzz: %d iterations, %d decoded, %d rejected\n", iterations, ok, rejected);
    return 0;
}

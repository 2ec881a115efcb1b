// exif_fuzz_main.cpp -- mutation fuzzer for the parser's Exif reader (jg_reader.cpp: note_exif_segment, exif_orientation),
// on files that carry the Exif segments of tests/exif_ref.py. Built with -fsanitize=address,undefined by
// tests/test_exif_fuzz_host.py: a read outside the file's buffer (an exact-size heap copy), a misaligned read or an
// overflow outside -fwrapv's reach aborts the run.
//
//   exif_fuzz_main <iterations> <seed> file.jpg [file.jpg ...]
//
// Three kinds of damage: bytes of the Exif data alone (TIFF header, offsets, counts, types: the parse must still SUCCEED --
// a bad Exif segment never fails parse_header -- with an orientation of 1..8); the APP1 marker's length field and the
// bytes around it; a truncated file. Every parse returns a status of the API, and exif_orientation alone is run on every
// prefix of the damaged data.
#include "jg_reader.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

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
    jg::Reader rd;
    jg::Logger log;
    int ok = 0, rejected = 0, oriented = 0;
    for (int it = 0; it < iterations; ++it) {
        const std::vector<uint8_t>& src = files[rnd() % files.size()];
        // the first Exif segment: [seg, seg + 2 + length) with the marker at seg
        size_t seg = 0, len = 0;
        for (size_t i = 2; i + 4 <= src.size() && src[i] == 0xFF && src[i + 1] != 0xDA;) {
            const size_t n = static_cast<size_t>(src[i + 2]) << 8 | src[i + 3];
            if (src[i + 1] == 0xE1 && n >= 8 && src[i + 4] == 'E') {
                seg = i;
                len = n;
                break;
            }
            i += 2 + n;
        }
        std::vector<uint8_t> d = src; // an exact-size heap copy: one byte too far is a report
        const int kind = seg == 0 ? 2 : static_cast<int>(rnd() % 3);
        bool must_parse = false;
        if (kind == 0 && len > 8) { // the data behind "Exif\0\0" only
            must_parse = true;
            for (int e = 1 + static_cast<int>(rnd() % 6); e > 0; --e) {
                const size_t pos = seg + 10 + rnd() % (len - 8);
                switch (rnd() % 5) {
                case 0: d[pos] = static_cast<uint8_t>(rnd()); break;
                case 1: d[pos] ^= static_cast<uint8_t>(1u << (rnd() % 8)); break;
                case 2: d[pos] = 0xFF; break; // offsets and counts at their largest
                case 3: d[pos] = 0; break;
                default: // the byte order flipped
                    d[seg + 10] = d[seg + 11] = d[seg + 10] == 'I' ? 'M' : 'I';
                }
            }
        } else if (kind == 1) { // the length field, the marker, the identifier
            for (int e = 1 + static_cast<int>(rnd() % 3); e > 0; --e) {
                const size_t pos = seg + rnd() % 10;
                d[pos]           = rnd() % 2 ? static_cast<uint8_t>(rnd()) : static_cast<uint8_t>(d[pos] ^ (1u << (rnd() % 8)));
            }
        } else if (d.size() > 8) {
            d.resize(2 + rnd() % (seg != 0 && rnd() % 2 ? seg + 2 + len : d.size() - 2)); // often inside the segment
            d.shrink_to_fit();
        }
        std::vector<uint8_t> exact(d.begin(), d.end());
        const jpeggpu_status st = rd.parse(exact.data(), exact.size(), 64, log, false, 0, 1, true);
        if (st < JPEGGPU_SUCCESS || st > JPEGGPU_INCOMPLETE_BITSTREAM) return 3;
        if (must_parse && st != JPEGGPU_SUCCESS) return 4; // a bad Exif segment never fails the parse
        if (st == JPEGGPU_SUCCESS) {
            if (rd.s.orientation < 1 || rd.s.orientation > 8) return 5;
            ++ok;
            oriented += rd.s.orientation != 1;
        } else {
            ++rejected;
        }
        if (seg != 0 && seg + 4 <= d.size()) { // the Exif reader alone, on every prefix of the damaged data
            const size_t n = d.size() - (seg + 4) < len - 2 ? d.size() - (seg + 4) : len - 2;
            for (size_t cut = 0; cut <= n; ++cut) {
                std::vector<uint8_t> part(d.begin() + seg + 4, d.begin() + seg + 4 + cut);
                const int o = jg::exif_orientation(part.data(), part.size());
                if (o < 1 || o > 8) return 6;
            }
        }
    }
    std::printf("exif fuzz: %d iterations, %d parsed (%d with an orientation), %d rejected\n", iterations, ok, oriented, rejected);
    return 0;
}

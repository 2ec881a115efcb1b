// encode_plan_check_main.cpp -- the encoder's host plan (jg_encode_plan.cpp) under AddressSanitizer + UBSan, without a
// device: where caller-supplied sizes, counts and frames become offsets into the staged blob and memcpy sizes. Built by
// tests/test_encode_plan_host.py from this file and jg_encode_plan.cpp alone; the two functions of the decoder's side that
// the plan's exports call (transcode_spec, coefficient_spec) hand out the synthetic spec below.
//
// The sweep. Every call carries the status it must return. An accepted call is planned, its blob is filled into a heap
// buffer of exactly plan.blob_bytes (an overrun is a sanitizer report), and then
//   * every offset of Plan, ProgPlan and each Item is a multiple of 256 (headers: 16);
//   * the regions ascend without overlap, the staged ones inside blob_bytes, the device's inside total;
//   * each header or OptState (with its long prefix) lies inside the blob's header region at its header_off;
//   * tile_start and chunk_start are the running sums, the sentinels close them, the shadow items' likewise;
//   * a transcode item's src and shadow_off point where the plan put them, a budget item's dqt_off inside its header;
//   * a scratch-size query and the full plan agree on `total`; planning and filling twice gives the same bytes.
// Prints per group of calls a SHA-256 over its calls' digests (blob, Plan, headers) -- the caller's pointers are constants,
// so they are the same in every run -- and the calls per kind; the exit status is the number of the check that failed.
#include "jg_encode_plan.hpp"

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

using namespace jg::enc;

namespace {

// ---- SHA-256 (FIPS 180-4) --------------------------------------------------------------------------
struct Sha256 {
    uint32_t h[8] = {0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19};
    uint8_t buf[64];
    uint64_t len = 0;
    static uint32_t ror(uint32_t x, int n) { return x >> n | x << (32 - n); }
    void block(const uint8_t* p)
    {
        static const uint32_t k[64] = {
            0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01, 0x243185be,
            0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc, 0x2de92c6f, 0x4a7484aa,
            0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147, 0x06ca6351, 0x14292967, 0x27b70a85,
            0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85, 0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3,
            0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08, 0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f,
            0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208, 0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2};
        uint32_t w[64], a[8];
        for (int i = 0; i < 16; ++i) w[i] = uint32_t(p[4 * i]) << 24 | uint32_t(p[4 * i + 1]) << 16 | uint32_t(p[4 * i + 2]) << 8 | p[4 * i + 3];
        for (int i = 16; i < 64; ++i)
            w[i] = w[i - 16] + (ror(w[i - 15], 7) ^ ror(w[i - 15], 18) ^ w[i - 15] >> 3) + w[i - 7] + (ror(w[i - 2], 17) ^ ror(w[i - 2], 19) ^ w[i - 2] >> 10);
        std::memcpy(a, h, sizeof a);
        for (int i = 0; i < 64; ++i) {
            const uint32_t t1 = a[7] + (ror(a[4], 6) ^ ror(a[4], 11) ^ ror(a[4], 25)) + ((a[4] & a[5]) ^ (~a[4] & a[6])) + k[i] + w[i];
            const uint32_t t2 = (ror(a[0], 2) ^ ror(a[0], 13) ^ ror(a[0], 22)) + ((a[0] & a[1]) ^ (a[0] & a[2]) ^ (a[1] & a[2]));
            for (int j = 7; j > 0; --j) a[j] = a[j - 1];
            a[4] += t1;
            a[0] = t1 + t2;
        }
        for (int i = 0; i < 8; ++i) h[i] += a[i];
    }
    void add(const void* data, size_t n)
    {
        const uint8_t* p = static_cast<const uint8_t*>(data);
        for (size_t i = 0; i < n; ++i) {
            buf[len++ % 64] = p[i];
            if (len % 64 == 0) block(buf);
        }
    }
    std::string hex()
    {
        const uint64_t bits = len * 8;
        const uint8_t one = 0x80, zero = 0;
        add(&one, 1);
        while (len % 64 != 56) add(&zero, 1);
        uint8_t be[8];
        for (int i = 0; i < 8; ++i) be[i] = uint8_t(bits >> (56 - 8 * i));
        add(be, 8);
        char out[65];
        for (int i = 0; i < 8; ++i) std::snprintf(out + 8 * i, 9, "%08x", h[i]);
        return out;
    }
};

// ---- cases and their counts ------------------------------------------------------------------------
char g_case[256] = "";
[[noreturn]] void fail(int code, const char* what)
{
    std::fprintf(stderr, "encode plan check: %s: %s\n", g_case, what);
    std::exit(code);
}
void need(bool ok, int code, const char* what)
{
    if (!ok) fail(code, what);
}
void begin(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
void begin(const char* fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_case, sizeof g_case, fmt, ap);
    va_end(ap);
}

enum Kind { kPixel, kCalls, kBudget, kLayout, kFrame, kRefused, kKinds };
const char* const kKindName[kKinds] = {"pixel items", "calls", "budget calls", "encoder-layout specs", "frame specs", "refused"};
int g_done[kKinds] = {};
Sha256 g_group;
void end_group(const char* name)
{
    std::printf("digest %s %s\n", name, g_group.hex().c_str());
    g_group = Sha256();
}

// the caller's pointers: constants, never dereferenced
uint8_t* const kBase = reinterpret_cast<uint8_t*>(uintptr_t{0x7000} << 24);
uint8_t* const kData = reinterpret_cast<uint8_t*>(uintptr_t{0x3000} << 24);
uint8_t* const kOut  = reinterpret_cast<uint8_t*>(uintptr_t{0x5000} << 24);
uint8_t* const kTmp  = reinterpret_cast<uint8_t*>(uintptr_t{0x6000} << 24);

jpeggpu_ext_encode_item pixel_item(int w, int h, int channels, int subsampling, int restart, int quality, int optimize, int progressive, int slot = 0)
{
    jpeggpu_ext_encode_item it{};
    it.data = kData + (size_t(slot) << 20), it.width = w, it.height = h, it.channels = channels, it.progressive = progressive;
    it.row_pitch = int64_t(w) * channels + 5, it.pixel_stride = channels, it.channel_stride = 1;
    it.quality = quality, it.subsampling = jpeggpu_ext_subsampling(subsampling), it.restart_interval = restart, it.optimize = optimize;
    it.out = kOut + (size_t(slot) << 20), it.capacity = 1000 + size_t(slot);
    return it;
}

/// A spec as transcode_spec makes it. `factors`: h, v per component as coded; null: one of the encoder's layouts, by the
/// item's subsampling. `wide`: the first `wide` tables hold 16-bit entries.
TranscodeSpec make_spec(const jpeggpu_ext_encode_item& item, const int (*factors)[2], int color_space, int tables, int wide, unsigned select, bool oriented)
{
    TranscodeSpec s{};
    s.item      = item;
    s.item.data = nullptr;
    const int n = item.channels;
    for (int t = 0; t < 2; ++t)
        for (int k = 0; k < 64; ++k) s.qtable[t][k] = uint8_t(1 + (k * 3 + t * 7 + item.width) % 255);
    const int hs = item.subsampling != JPEGGPU_EXT_SUBSAMPLING_444 ? 2 : 1, vs = item.subsampling == JPEGGPU_EXT_SUBSAMPLING_420 ? 2 : 1;
    s.sampling0 = uint8_t(hs << 4 | vs);
    for (int c = 0; c < n; ++c) {
        GatherComp& g = s.src.comp[c];
        g.sym = reinterpret_cast<const uint16_t*>(kTmp + 4096 * c), g.du_tab = kTmp + 65536 + 4096 * c, g.sym_limit = 1000 + c;
        g.du_per_mcu = 3, g.k0 = c, g.h = g.v = 1, g.mcus_x = (item.width + 7) / 8;
        g.vis_x = g.dst_x = (item.width + 7) / 8, g.vis_y = g.dst_y = (item.height + 7) / 8;
    }
    s.src.uncodable = 77; // (the fill zeroes it)
    s.src.oriented = oriented, s.src.mirror_x = oriented;
    if (!factors) return s;
    s.general     = true;
    s.color_space = color_space;
    s.tables_n    = tables;
    for (int t = 0; t < tables; ++t) {
        s.table_id[t] = uint8_t(t), s.table16[t] = t < wide;
        for (int k = 0; k < 64; ++k) s.table[t][k] = uint16_t(1 + (k * 5 + t) % 255 + (t < wide && k == 63 ? 4000 : 0));
    }
    Frame& f = s.frame;
    f.ncomp  = uint8_t(n);
    int hmax = 1, vmax = 1, j = 0;
    for (int c = 0; c < n; ++c) hmax = factors[c][0] > hmax ? factors[c][0] : hmax, vmax = factors[c][1] > vmax ? factors[c][1] : vmax;
    for (int c = 0; c < n; ++c) {
        const int h = n == 1 ? 1 : factors[c][0], v = n == 1 ? 1 : factors[c][1]; // a single component's MCU is one block
        s.comp[c].id = uint8_t(color_space == JPEGGPU_EXT_COLOR_CMYK ? "CMYK"[c] : c + 1), s.comp[c].h = uint8_t(factors[c][0]), s.comp[c].v = uint8_t(factors[c][1]);
        s.comp[c].tq = uint8_t(c % tables), s.comp[c].select = select >> c & 1;
        for (int yo = 0; yo < v; ++yo)
            for (int xo = 0; xo < h; ++xo, ++j) f.map |= uint64_t(c | xo << 2 | yo << 4) << (6 * j), f.last |= uint64_t(h * v - 1) << (4 * j);
        f.hv |= uint32_t(h | v << 4) << (8 * c);
        f.select |= uint8_t(s.comp[c].select << c);
        f.grid_w[c] = n == 1 ? (item.width + 7) / 8 : ((item.width * h + hmax - 1) / hmax + 7) / 8;
        f.grid_h[c] = n == 1 ? (item.height + 7) / 8 : ((item.height * v + vmax - 1) / vmax + 7) / 8;
    }
    if (j > kMaxMcuBlocks) fail(3, "a synthetic frame beyond kMaxMcuBlocks");
    return s;
}

/// Plan's fields (the struct has four bytes of padding behind `oriented`).
std::string plan_digest(const Plan& p)
{
    Sha256 d;
    d.add(&p.n, sizeof p.n), d.add(&p.optimized, sizeof p.optimized), d.add(&p.oriented, sizeof p.oriented);
    d.add(&p.prog, sizeof p.prog);
    d.add(&p.tiles, sizeof p - offsetof(Plan, tiles));
    return d.hex();
}

struct Region {
    uint64_t off, bytes;
    const char* name;
};

/// Plans the call, expects `want`; an accepted call is filled and checked, and its digests join the group's.
void check_call(Kind kind, const jpeggpu_ext_encode_item* items, const TranscodeSpec* specs, int n, const jpeggpu_ext_encode_fit_item* budgets, int want)
{
    ++g_done[kind];
    CallPlan call, query, again;
    const jpeggpu_status st = make_plan(items, specs, n, budgets != nullptr, false, call);
    if (st != want) {
        std::fprintf(stderr, "encode plan check: %s: status %d, expected %d\n", g_case, int(st), want);
        std::exit(2);
    }
    const jpeggpu_status sq = make_plan(items, specs, n, budgets != nullptr, true, query);
    need(sq == st, 4, "a scratch-size query and the full plan disagree on the status");
    if (st != JPEGGPU_SUCCESS) return;
    const Plan& p = call.plan;
    need(query.plan.total == p.total && query.plan.blob_bytes == p.blob_bytes, 5, "a scratch-size query and the full plan disagree on the sizes");
    need(scratch_size_of(items, specs, n, budgets != nullptr) == p.total + 256, 5, "scratch_size_of is not total + 256");
    std::unique_ptr<uint8_t[]> blob(new uint8_t[p.blob_bytes]), blob2(new uint8_t[p.blob_bytes]);
    fill_blob(call, items, specs, budgets, kBase, blob.get());
    need(make_plan(items, specs, n, budgets != nullptr, false, again) == JPEGGPU_SUCCESS, 6, "the second plan fails");
    fill_blob(again, items, specs, budgets, kBase, blob2.get());
    need(plan_digest(again.plan) == plan_digest(p) && std::memcmp(blob.get(), blob2.get(), p.blob_bytes) == 0, 6, "planning twice gives other bytes");

    // the plan's regions, in the order they were taken
    const uint64_t np = uint64_t(p.prog.n), tiles = p.tiles, chunks = p.chunks, pt = p.prog.tiles, pc = p.prog.chunks;
    need(p.n == n && p.items_off > p.tables_off, 7, "the plan's n");
    const uint64_t headers_off = p.items_off + (sizeof(Item) * (uint64_t(n) + 1) + 255) / 256 * 256;
    const Region staged[] = {{p.tables_off, sizeof(Tables), "tables"}, {p.items_off, sizeof(Item) * (uint64_t(n) + 1), "items"},
                             {headers_off, p.prog.shadow_off - headers_off, "headers"}, {p.prog.shadow_off, np ? sizeof(Item) * (np + 1) : 0, "shadow"},
                             {p.prog.items_off, sizeof(ProgItem) * np, "prog items"}, {p.gather_off, specs ? sizeof(GatherSrc) * uint64_t(n) : 0, "gather"},
                             {p.fit_off, budgets ? sizeof(FitItem) * uint64_t(n) : 0, "fit"}};
    const Region device[] = {{p.bits_off, tiles * kTileBlocks * 4, "bits"}, {p.tile_sum_off, tiles * sizeof(Cursor), "tile_sum"},
                             {p.tile_before_off, tiles * sizeof(Cursor), "tile_before"}, {p.count_off, chunks * sizeof(Count), "count"},
                             {p.count_before_off, chunks * sizeof(Count), "count_before"}, {p.prog.bits_off, pt * kTileBlocks * 4, "prog bits"},
                             {p.prog.facts_off, pt * kTileBlocks, "prog facts"}, {p.prog.eobn_off, pt * kTileBlocks * 2, "prog eobn"},
                             {p.prog.tile_sum_off, pt * sizeof(Cursor), "prog tile_sum"}, {p.prog.tile_before_off, pt * sizeof(Cursor), "prog tile_before"},
                             {p.prog.count_off, pc * sizeof(Count), "prog count"}, {p.prog.count_before_off, pc * sizeof(Count), "prog count_before"}};
    uint64_t end = 0;
    for (const Region& r : staged) {
        need(r.off % 256 == 0 && r.off >= end, 8, r.name);
        end = r.off + r.bytes;
        need(end <= p.blob_bytes, 8, r.name);
    }
    need(p.blob_bytes % 256 == 0 && p.total % 256 == 0 && p.blob_bytes <= p.total, 8, "blob_bytes and total");
    end = p.blob_bytes;
    for (const Region& r : device) {
        need(r.off % 256 == 0 && r.off >= end, 9, r.name);
        end = r.off + r.bytes;
        need(end <= p.total, 9, r.name);
    }

    // the items, as the device will read them
    std::vector<Item> dev(size_t(n) + 1), shadow(size_t(np ? np + 1 : 0));
    std::vector<ProgItem> prog(size_t(np), ProgItem{});
    std::memcpy(dev.data(), blob.get() + p.items_off, sizeof(Item) * dev.size());
    if (np) std::memcpy(shadow.data(), blob.get() + p.prog.shadow_off, sizeof(Item) * shadow.size());
    if (np) std::memcpy(prog.data(), blob.get() + p.prog.items_off, sizeof(ProgItem) * prog.size());
    Sha256 headers;
    uint64_t tile = 0, chunk = 0, ptile = 0, pchunk = 0, header_end = headers_off, k = 0;
    int optimized = 0;
    for (int i = 0; i < n; ++i) {
        const Item& d = dev[size_t(i)];
        need(d.coef_off % 256 == 0 && d.stream_off % 256 == 0 && d.starts_off % 256 == 0, 10, "an item's offsets are not multiples of 256");
        need(d.coef_off >= end && d.stream_off >= d.coef_off + uint64_t(d.blocks) * 128 && d.starts_off >= d.stream_off, 10, "an item's arrays overlap");
        const uint64_t chunks_i = (d.starts_off - d.stream_off) / kChunkBytes;
        need((d.starts_off - d.stream_off) % kChunkBytes == 0, 10, "an item's stream is not whole chunks");
        end = d.starts_off + chunks_i * (kChunkBytes / 8);
        need(end <= p.total, 10, "an item's arrays end beyond total");
        need(d.tile_start == tile && d.header_off % 16 == 0 && d.header_off >= header_end, 11, "an item's tile_start or header_off");
        tile += (uint64_t(d.blocks) + kTileBlocks - 1) / kTileBlocks;
        uint64_t work = 0, work_bytes = 0, header_bytes = 0;
        if (d.header_len == kProgressiveHeader) {
            need(k < np, 12, "more progressive items than the plan counts");
            const Item& sh = shadow[size_t(k)];
            const ProgItem& pi = prog[size_t(k)];
            need(sh.tile_start == ptile && sh.chunk_start == pchunk && sh.stream_off == d.stream_off && sh.out == d.out, 12, "a shadow item");
            need(pi.item == uint32_t(i) && pi.scans_n >= 6 && pi.scans_n <= uint32_t(kProgScans) && pi.slots_n <= uint32_t(kProgSlots) &&
                     pi.prefix_len <= sizeof pi.prefix && int(pi.slots_n) <= p.prog.slots,
                 12, "a ProgItem");
            uint64_t scan_blocks = 0;
            for (uint32_t s = 0; s < pi.scans_n; ++s) {
                need(pi.scans[s].first == scan_blocks && pi.scans[s].sos_len <= sizeof pi.scans[s].sos, 12, "a scan's first block or header");
                scan_blocks += uint64_t(pi.scans[s].blocks);
            }
            ptile += (scan_blocks + kTileBlocks - 1) / kTileBlocks;
            pchunk += chunks_i;
            work = pi.work_off, work_bytes = sizeof(ProgWork);
            if (specs) {
                GatherSrc g;
                std::memcpy(&g, blob.get() + p.gather_off + sizeof(GatherSrc) * size_t(i), sizeof g);
                need(g.shadow_off == p.prog.shadow_off + sizeof(Item) * k, 13, "a transcode item's shadow_off");
            }
            ++k;
        } else {
            need(d.chunk_start == chunk, 11, "an item's chunk_start");
            chunk += chunks_i;
            header_bytes = d.header_len;
            if (d.header_len == 0) {
                OptState st;
                need(d.header_off + sizeof st <= p.prog.shadow_off, 14, "an OptState ends beyond the headers");
                std::memcpy(&st, blob.get() + d.header_off, sizeof st);
                header_bytes = sizeof st + (long_prefix(st.prefix_len) ? st.prefix_len : 0);
                need(st.prefix_len <= uint32_t(kLongPrefixBytes) && st.suffix_len <= sizeof st.suffix, 14, "an OptState's lengths");
                work = st.work_off, work_bytes = sizeof(OptWork);
                ++optimized;
            }
            need(d.header_off + header_bytes <= p.prog.shadow_off, 14, "a header ends beyond the headers");
            headers.add(blob.get() + d.header_off, header_bytes);
            header_end = d.header_off + header_bytes;
        }
        if (work_bytes) {
            need(work % 256 == 0 && work >= end && work + work_bytes <= p.total, 15, "an item's work area");
            end = work + work_bytes;
        }
        if (specs) need(d.src == kBase + p.gather_off + sizeof(GatherSrc) * size_t(i), 13, "a transcode item's src");
        if (budgets) {
            FitItem f;
            std::memcpy(&f, blob.get() + p.fit_off + sizeof f * size_t(i), sizeof f);
            need(f.raw_off % 256 == 0 && f.raw_off >= end && f.raw_off + uint64_t(d.blocks) * 128 <= p.total && f.blocks == d.blocks, 16, "a budget item's transform");
            end = f.raw_off + uint64_t(d.blocks) * 128;
            need(f.dqt_off[0] > d.header_off && (d.channels == 1 ? f.dqt_off[1] == 0 : f.dqt_off[1] > f.dqt_off[0] + 64), 16, "a budget item's dqt_off");
            for (int t = 0; t < 2; ++t) need(!f.dqt_off[t] || (f.dqt_off[t] + 64 <= header_end && blob[f.dqt_off[t] - 1] == t), 16, "dqt_off is not a DQT payload");
            need(f.lo == budgets[i].quality_min && f.hi == budgets[i].quality_max && f.q == f.hi && f.max_bytes == budgets[i].max_bytes, 16, "a budget item's range");
        }
    }
    need(dev[size_t(n)].tile_start == tile && dev[size_t(n)].chunk_start == chunk && tile == tiles && chunk == chunks, 17, "the sentinel does not close the sums");
    need(k == np && optimized == p.optimized && (!np || (shadow[size_t(np)].tile_start == ptile && shadow[size_t(np)].chunk_start == pchunk)) && ptile == pt &&
             pchunk == pc,
         17, "the progressive sentinel does not close the sums");
    need(end <= p.total, 17, "total");

    Sha256 b;
    b.add(blob.get(), p.blob_bytes);
    const std::string line = b.hex() + plan_digest(p) + headers.hex();
    g_group.add(line.data(), line.size());
}

const int kLen[] = {1, 7, 8, 9, 15, 16, 17, 33};
const int kRestart[] = {0, 1, 2, 65535};
const int kQuality[] = {1, 50, 100};

void pixel_items()
{
    for (int mode = 0; mode < 4; ++mode)
        for (int channels = 1; channels <= 3; channels += 2)
            for (int sub = 0; sub < 3; ++sub) {
                for (int s = 0; s < 66; ++s) {
                    const int w = s < 64 ? kLen[s / 8] : s == 64 ? 65535 : 1, h = s < 64 ? kLen[s % 8] : s == 64 ? 1 : 65535;
                    for (int restart : kRestart)
                        for (int quality : kQuality) {
                            begin("pixel %dx%d ch %d sub %d restart %d q %d mode %d", w, h, channels, sub, restart, quality, mode);
                            const jpeggpu_ext_encode_item it = pixel_item(w, h, channels, sub, restart, quality, mode & 1, mode >> 1);
                            check_call(kPixel, &it, nullptr, 1, nullptr, JPEGGPU_SUCCESS);
                        }
                }
                char name[64];
                std::snprintf(name, sizeof name, "pixel_o%d_p%d_c%d_s%d", mode & 1, mode >> 1, channels, sub);
                end_group(name);
            }
}

/// Calls of 1, 2 and 5 items mixing the kinds (0 plain, 1 optimised, 2 progressive, 3 both), as plain and as budget calls.
void calls()
{
    const int mixes[][5] = {{0, 1, -1}, {2, 3, -1}, {1, 0, 2, 0, 1}, {0, 2, 3, 1, 0}, {2, 2, 2, 3, 3}, {0, 0, 0, 0, 0}, {1, -1}, {3, -1}};
    for (const auto& mix : mixes)
        for (int v = 0; v < 6; ++v) {
            jpeggpu_ext_encode_item items[5];
            jpeggpu_ext_encode_fit_item fit[5];
            int n = 0;
            bool progressive = false;
            for (; n < 5 && mix[n] >= 0; ++n) {
                items[n] = pixel_item(kLen[(v + 3 * n) % 8] + 16 * (n % 2), kLen[(2 * v + n) % 8], (v + n) % 2 ? 3 : 1, (v + n) % 3, kRestart[(v + n) % 4], kQuality[v % 3], mix[n] & 1, mix[n] >> 1, n);
                progressive |= mix[n] >> 1;
                fit[n] = jpeggpu_ext_encode_fit_item{items[n], size_t(500 + 100 * n), 1 + v, 100 - n};
            }
            begin("call of %d items, mix %d.., variant %d", n, mix[0], v);
            check_call(kCalls, items, nullptr, n, nullptr, JPEGGPU_SUCCESS);
            if (!progressive) check_call(kBudget, items, nullptr, n, fit, JPEGGPU_SUCCESS); // (jg_encode_fit.cpp refuses the others before the plan)
        }
    end_group("calls");
}

const int kF1[][2] = {{1, 1}}, kF1b[][2] = {{2, 2}}, kF2[][2] = {{2, 1}, {1, 1}}, kF3a[][2] = {{2, 2}, {1, 1}, {1, 1}}, kF3b[][2] = {{4, 1}, {1, 1}, {1, 1}},
          kF3c[][2] = {{2, 2}, {2, 1}, {1, 2}}, kF3d[][2] = {{4, 2}, {1, 1}, {1, 1}}, kF3e[][2] = {{1, 2}, {1, 1}, {1, 1}}, kF4a[][2] = {{1, 1}, {1, 1}, {1, 1}, {1, 1}},
          kF4b[][2] = {{2, 2}, {1, 1}, {1, 1}, {2, 2}};
const struct {
    int n;
    const int (*factors)[2];
} kFrames[] = {{1, kF1}, {1, kF1b}, {2, kF2}, {3, kF3a}, {3, kF3b}, {3, kF3c}, {3, kF3d}, {3, kF3e}, {4, kF4a}, {4, kF4b}};
const int kColors[] = {JPEGGPU_EXT_COLOR_GRAY, JPEGGPU_EXT_COLOR_YCBCR, JPEGGPU_EXT_COLOR_RGB, JPEGGPU_EXT_COLOR_CMYK, JPEGGPU_EXT_COLOR_YCCK, JPEGGPU_EXT_COLOR_UNKNOWN};

void spec_calls()
{
    const int sizes[][2] = {{1, 1}, {17, 9}, {33, 16}, {65535, 1}, {1, 65535}};
    for (int mode = 0; mode < 4; ++mode)
        for (const auto& size : sizes)
            for (int channels = 1; channels <= 3; channels += 2)
                for (int sub = 0; sub < 3; ++sub)
                    for (int restart : kRestart) {
                        begin("encoder-layout spec %dx%d ch %d sub %d restart %d mode %d", size[0], size[1], channels, sub, restart, mode);
                        const TranscodeSpec s = make_spec(pixel_item(size[0], size[1], channels, sub, restart, 75, mode & 1, mode >> 1), nullptr, 0, 0, 0, 0, restart == 2);
                        check_call(kLayout, &s.item, &s, 1, nullptr, JPEGGPU_SUCCESS);
                    }
    end_group("encoder_layout_specs");
    for (const auto& frame : kFrames) {
        for (int mode = 0; mode < 4; ++mode)
            for (int color : kColors)
                for (int tables = 1; tables <= 4; ++tables)
                    for (int wide = 0; wide <= tables; wide += tables) // none or all of them 16-bit: four wide ones with optimise reach the long prefix
                        for (int sel = 0; sel < 3; ++sel)
                            for (int size = 0; size < 3; ++size) {
                                const unsigned select = sel == 0 ? 0u : sel == 1 ? 15u : 6u;
                                begin("frame spec of %d components (%dx%d first), colour %d, %d tables (%d wide), select %u, mode %d, size %d", frame.n,
                                      frame.factors[0][0], frame.factors[0][1], color, tables, wide, select, mode, size);
                                const jpeggpu_ext_encode_item it = pixel_item(sizes[size][0], sizes[size][1], frame.n, 0, kRestart[(tables + sel) % 4], 75, mode & 1, mode >> 1);
                                const TranscodeSpec s = make_spec(it, frame.factors, color, tables, wide, select & ((1u << frame.n) - 1), size == 1);
                                check_call(kFrame, &s.item, &s, 1, nullptr, JPEGGPU_SUCCESS);
                            }
        char name[64];
        std::snprintf(name, sizeof name, "frame_specs_%d_of_%d_components", int(&frame - kFrames), frame.n);
        end_group(name);
    }
    // calls of several transcode items: the two kinds of spec and every option side by side
    for (int v = 0; v < 8; ++v) {
        std::vector<TranscodeSpec> specs;
        std::vector<jpeggpu_ext_encode_item> items;
        for (int i = 0; i < 5; ++i) {
            const auto& frame = kFrames[(v + 2 * i) % 10];
            const int mode = (v + i) % 4;
            if (i % 2) specs.push_back(make_spec(pixel_item(17 + v, 9 + i, i == 1 ? 1 : 3, (v + i) % 3, kRestart[i % 4], 75, mode & 1, mode >> 1, i), nullptr, 0, 0, 0, 0, v % 2));
            else specs.push_back(make_spec(pixel_item(33 - v, 16 + i, frame.n, 0, kRestart[(v + i) % 4], 75, mode & 1, mode >> 1, i), frame.factors, kColors[(v + i) % 6], 1 + (v + i) % 4, v % 2 ? 1 + (v + i) % 4 : 0, 6u & ((1u << frame.n) - 1), i == 2));
            items.push_back(specs.back().item);
        }
        for (int n : {2, 5}) {
            begin("transcode call %d of %d items", v, n);
            check_call(kFrame, items.data(), specs.data(), n, nullptr, JPEGGPU_SUCCESS);
        }
    }
    end_group("transcode_calls");
}

TranscodeSpec g_spec; // what transcode_spec and coefficient_spec hand out

void refused()
{
    const jpeggpu_ext_encode_item good = pixel_item(17, 9, 3, 2, 2, 50, 0, 0);
    size_t size = 0;
    begin("null pointers and item counts");
    check_call(kRefused, nullptr, nullptr, 1, nullptr, JPEGGPU_INVALID_ARGUMENT);
    check_call(kRefused, &good, nullptr, 0, nullptr, JPEGGPU_INVALID_ARGUMENT);
    check_call(kRefused, &good, nullptr, -1, nullptr, JPEGGPU_INVALID_ARGUMENT);
    check_call(kRefused, &good, nullptr, 65536, nullptr, JPEGGPU_INVALID_ARGUMENT);
    need(jpeggpu_ext_encode_header(nullptr, nullptr, &size) == JPEGGPU_INVALID_ARGUMENT && jpeggpu_ext_encode_header(&good, nullptr, nullptr) == JPEGGPU_INVALID_ARGUMENT, 20, "header: null");
    need(jpeggpu_ext_encode_bound(nullptr) == 0 && jpeggpu_ext_encode_scratch_size(nullptr, 1) == 0 && jpeggpu_ext_encode_scratch_size(&good, 0) == 0, 20, "bound, scratch: null");
    need(jpeggpu_ext_transcode_header(nullptr, nullptr, &size) == JPEGGPU_INVALID_ARGUMENT && jpeggpu_ext_transcode_bound(nullptr) == 0 &&
             jpeggpu_ext_transcode_scratch_size(nullptr, 1) == 0 && jpeggpu_ext_write_coefficients_header(nullptr, nullptr, &size) == JPEGGPU_INVALID_ARGUMENT &&
             jpeggpu_ext_write_coefficients_bound(nullptr) == 0 && jpeggpu_ext_write_coefficients_scratch_size(nullptr, 1) == 0,
         20, "the spec calls: null");
    // every field one step outside its range, alone and behind a good item
    struct Edit {
        const char* name;
        void (*apply)(jpeggpu_ext_encode_item&);
    };
    const Edit edits[] = {{"width 0", [](jpeggpu_ext_encode_item& it) { it.width = 0; }},       {"width 65536", [](jpeggpu_ext_encode_item& it) { it.width = 65536; }},
                          {"height 0", [](jpeggpu_ext_encode_item& it) { it.height = 0; }},     {"height 65536", [](jpeggpu_ext_encode_item& it) { it.height = 65536; }},
                          {"channels 0", [](jpeggpu_ext_encode_item& it) { it.channels = 0; }}, {"channels 2", [](jpeggpu_ext_encode_item& it) { it.channels = 2; }},
                          {"channels 4", [](jpeggpu_ext_encode_item& it) { it.channels = 4; }}, {"quality 0", [](jpeggpu_ext_encode_item& it) { it.quality = 0; }},
                          {"quality 101", [](jpeggpu_ext_encode_item& it) { it.quality = 101; }},
                          {"subsampling -1", [](jpeggpu_ext_encode_item& it) { it.subsampling = jpeggpu_ext_subsampling(-1); }},
                          {"subsampling 3", [](jpeggpu_ext_encode_item& it) { it.subsampling = jpeggpu_ext_subsampling(3); }},
                          {"restart -1", [](jpeggpu_ext_encode_item& it) { it.restart_interval = -1; }},
                          {"restart 65536", [](jpeggpu_ext_encode_item& it) { it.restart_interval = 65536; }},
                          {"optimize -1", [](jpeggpu_ext_encode_item& it) { it.optimize = -1; }},       {"optimize 2", [](jpeggpu_ext_encode_item& it) { it.optimize = 2; }},
                          {"progressive -1", [](jpeggpu_ext_encode_item& it) { it.progressive = -1; }}, {"progressive 2", [](jpeggpu_ext_encode_item& it) { it.progressive = 2; }}};
    for (const Edit& e : edits) {
        begin("refused: %s", e.name);
        jpeggpu_ext_encode_item two[2] = {good, good};
        e.apply(two[1]);
        check_call(kRefused, two + 1, nullptr, 1, nullptr, JPEGGPU_INVALID_ARGUMENT);
        check_call(kRefused, two, nullptr, 2, nullptr, JPEGGPU_INVALID_ARGUMENT);
        need(jpeggpu_ext_encode_header(two + 1, nullptr, &size) == JPEGGPU_INVALID_ARGUMENT && jpeggpu_ext_encode_bound(two + 1) == 0 &&
                 jpeggpu_ext_encode_scratch_size(two, 2) == 0,
             21, "the exports accept it");
    }
    for (int channels : {0, 5}) { // a frame of its own has one to four components
        begin("refused: a frame spec of %d components", channels);
        TranscodeSpec s = make_spec(pixel_item(17, 9, 3, 0, 0, 75, 0, 0), kF3a, JPEGGPU_EXT_COLOR_YCBCR, 2, 0, 6, false);
        s.item.channels = channels;
        check_call(kRefused, &s.item, &s, 1, nullptr, JPEGGPU_INVALID_ARGUMENT);
    }
    for (int mode = 0; mode < 4; ++mode) {
        begin("refused: 65535 x 65535, mode %d", mode);
        jpeggpu_ext_encode_item big[2] = {pixel_item(65535, 65535, 3, 0, 0, 50, mode & 1, mode >> 1), good};
        check_call(kRefused, big, nullptr, 1, nullptr, JPEGGPU_NOT_SUPPORTED);
        size = 0;
        need(jpeggpu_ext_encode_scratch_size(big, 1) == 0 && jpeggpu_ext_encode_bound(big) > 0, 22, "the exports at 65535 x 65535");
        big[1].quality = 0; // an invalid item behind it is what the call reports
        check_call(kRefused, big, nullptr, 2, nullptr, JPEGGPU_INVALID_ARGUMENT);
    }
    {   // items that fit one by one and whose summed tiles reach 2^31 (a call's chunks cannot before its tiles do: an item
        // of the most chunks, 65536, has some 10000 tiles, and a call has at most 65535 items)
        begin("refused: summed tiles");
        std::vector<jpeggpu_ext_encode_item> many(45000, pixel_item(12000, 12000, 1, 0, 0, 50, 0, 0)); // 8790 tiles each
        check_call(kRefused, many.data(), nullptr, 1, nullptr, JPEGGPU_SUCCESS);
        check_call(kRefused, many.data(), nullptr, 954, nullptr, JPEGGPU_SUCCESS);
        check_call(kRefused, many.data(), nullptr, 955, nullptr, JPEGGPU_NOT_SUPPORTED);
        begin("refused: summed tiles of progressive items");
        for (auto& it : many) it = pixel_item(8, 65535, 1, 0, 0, 50, 0, 1); // 8192 blocks in six scans: 192 tiles each, counted apart
        CallPlan q;
        need(make_plan(many.data(), nullptr, 43690, false, true, q) == JPEGGPU_SUCCESS && make_plan(many.data(), nullptr, 43691, false, true, q) == JPEGGPU_NOT_SUPPORTED,
             23, "43690 tall progressive items fit, one more does not");
        ++g_done[kRefused];
    }
    // the spec calls through the synthetic spec: the header as the plain call's, bound and scratch as planned
    for (int optimize = 0; optimize < 2; ++optimize) {
        begin("the spec exports, optimize %d", optimize);
        g_spec = make_spec(pixel_item(33, 17, 4, 0, 2, 75, optimize, 0), kF4b, JPEGGPU_EXT_COLOR_CMYK, 4, 4, 0, false);
        jpeggpu_ext_transcode_item t{};
        jpeggpu_ext_coefficient_item c{};
        uint8_t head[1024];
        size_t a = sizeof head, b = sizeof head;
        const jpeggpu_status want = optimize ? JPEGGPU_NOT_SUPPORTED : JPEGGPU_SUCCESS;
        need(jpeggpu_ext_transcode_header(&t, head, &a) == want && jpeggpu_ext_write_coefficients_header(&c, head, &b) == want && a == b && a > 4 * 133, 24, "header");
        need(jpeggpu_ext_transcode_bound(&t) > a && jpeggpu_ext_transcode_bound(&t) == jpeggpu_ext_write_coefficients_bound(&c), 24, "bound");
        need(jpeggpu_ext_transcode_scratch_size(&t, 1) == scratch_size_of(&g_spec.item, &g_spec, 1, false) && jpeggpu_ext_write_coefficients_scratch_size(&c, 1) > 0, 24, "scratch size");
        ++g_done[kRefused];
    }
}

} // namespace

namespace jg {
namespace enc {
jpeggpu_status transcode_spec(const jpeggpu_ext_transcode_item&, bool, TranscodeSpec& spec)
{
    spec = g_spec;
    return JPEGGPU_SUCCESS;
}
jpeggpu_status coefficient_spec(const jpeggpu_ext_coefficient_item&, bool, TranscodeSpec& spec)
{
    spec = g_spec;
    return JPEGGPU_SUCCESS;
}
} // namespace enc
} // namespace jg

int main()
{
    pixel_items();
    calls();
    spec_calls();
    refused();
    std::printf("encode plan check:");
    for (int k = 0; k < kKinds; ++k) std::printf(" %d %s%s", g_done[k], kKindName[k], k + 1 < kKinds ? "," : "\n");
    return 0;
}

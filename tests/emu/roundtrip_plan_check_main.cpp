// roundtrip_plan_check_main.cpp -- the round trip's host plan (jg_roundtrip_plan.cpp, with jg_output_plan.cpp for its second
// stage) in a stand-alone program, built with -fsanitize=address,undefined by tests/test_roundtrip_plan_host.py. It plans
// calls without a device: every refusal, the tile starts at the tile size's edges, the scratch layout, and the fill of the
// staged bytes into a heap buffer of exactly the plan's size. It prints each item geometry and quantisation table it is asked
// for, which the test compares with tests/encode_ref.py.
//
//   roundtrip_plan_check_main                       the checks; "roundtrip plan check: N checks passed" and exit status 0
//   roundtrip_plan_check_main W H CHANNELS SUBSAMPLING QUALITY ...   one line per five arguments:
//                                                   "hs vs mcus_x mcus_y grid_w grid_h blocks | 64 luma | 64 chroma"
#include "jg_roundtrip_plan.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

namespace {

int g_checks = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        ++g_checks;                                                              \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                        \
        }                                                                        \
    } while (0)

uint8_t* const kBase = reinterpret_cast<uint8_t*>(uintptr_t{1} << 40); // 256-aligned, never dereferenced
uint8_t* const kSrc  = reinterpret_cast<uint8_t*>(uintptr_t{2} << 40);
uint8_t* const kDst  = reinterpret_cast<uint8_t*>(uintptr_t{3} << 40);

jpeggpu_ext_roundtrip_item rgb(int w, int h, int quality = 75, int ss = JPEGGPU_EXT_SUBSAMPLING_420)
{
    return jpeggpu_ext_roundtrip_item{kSrc, w, h, 3, int64_t{3} * w, 3, 1, quality, ss, kDst, 3 * w, 0};
}
jpeggpu_ext_roundtrip_item grey(int w, int h, int quality = 75)
{
    return jpeggpu_ext_roundtrip_item{kSrc, w, h, 1, w, 1, 0, quality, -7 /* not read for grey */, kDst, w, 0};
}

jpeggpu_status plan(const std::vector<jpeggpu_ext_roundtrip_item>& items, int layout, jg::rt::Plan& p)
{
    return jg::rt::plan_roundtrip(items.data(), static_cast<int>(items.size()), layout, kBase, p);
}
jpeggpu_status plan1(const jpeggpu_ext_roundtrip_item& it, int layout = JPEGGPU_EXT_HWC)
{
    jg::rt::Plan p;
    return plan({it}, layout, p);
}

/// The staged bytes in a heap buffer of exactly their size (ASan sees a byte too many), twice: the fill is deterministic.
void check_fill(const jg::rt::Plan& p)
{
    std::unique_ptr<uint8_t[]> a(new uint8_t[p.head]), b(new uint8_t[p.head]);
    std::memset(a.get(), 0xA5, p.head);
    std::memset(b.get(), 0x5A, p.head);
    jg::rt::fill_roundtrip(p, a.get());
    jg::rt::fill_roundtrip(p, b.get());
    CHECK(std::memcmp(a.get(), b.get(), p.head) == 0);
    CHECK(std::memcmp(a.get() + p.off_items, p.items.data(), sizeof(jg::rt::Item) * p.items.size()) == 0);
}

void check_refusals()
{
    const int HWC = JPEGGPU_EXT_HWC, CHW = JPEGGPU_EXT_CHW;
    jg::rt::Plan p;
    CHECK(plan1(rgb(17, 9)) == JPEGGPU_SUCCESS && plan1(grey(17, 9)) == JPEGGPU_SUCCESS);
    CHECK(jg::rt::plan_roundtrip(nullptr, 1, HWC, kBase, p) == JPEGGPU_INVALID_ARGUMENT);
    const jpeggpu_ext_roundtrip_item one = rgb(8, 8);
    for (int n : {0, -1, 65536}) CHECK(jg::rt::plan_roundtrip(&one, n, HWC, kBase, p) == JPEGGPU_INVALID_ARGUMENT);
    for (int n : {0, -1, 65536}) CHECK(jpeggpu_ext_roundtrip_scratch_size(&one, n) == 0);
    CHECK(jpeggpu_ext_roundtrip_scratch_size(nullptr, 1) == 0);
    for (int layout : {-1, 2}) CHECK(plan1(one, layout) == JPEGGPU_INVALID_ARGUMENT);
    jpeggpu_ext_roundtrip_item it;
    it = one, it.data = nullptr;
    CHECK(plan1(it) == JPEGGPU_INVALID_ARGUMENT);
    it = one, it.dst = nullptr;
    CHECK(plan1(it) == JPEGGPU_INVALID_ARGUMENT);
    for (int side : {0, -1, 65536}) {
        it = one, it.width = side;
        CHECK(plan1(it) == JPEGGPU_INVALID_ARGUMENT && jpeggpu_ext_roundtrip_scratch_size(&it, 1) == 0);
        it = one, it.height = side;
        CHECK(plan1(it) == JPEGGPU_INVALID_ARGUMENT && jpeggpu_ext_roundtrip_scratch_size(&it, 1) == 0);
    }
    for (int ch : {0, 2, 4}) {
        it = one, it.channels = ch;
        CHECK(plan1(it) == JPEGGPU_INVALID_ARGUMENT && jpeggpu_ext_roundtrip_scratch_size(&it, 1) == 0);
    }
    for (int q : {0, -1, 101}) {
        it = one, it.quality = q;
        CHECK(plan1(it) == JPEGGPU_INVALID_ARGUMENT && jpeggpu_ext_roundtrip_scratch_size(&it, 1) == 0);
        it = grey(8, 8, q);
        CHECK(plan1(it) == JPEGGPU_INVALID_ARGUMENT);
    }
    for (int ss : {-1, 3}) {
        it = one, it.subsampling = ss;
        CHECK(plan1(it) == JPEGGPU_INVALID_ARGUMENT && jpeggpu_ext_roundtrip_scratch_size(&it, 1) == 0);
    }
    // pitches: HWC 3 w, CHW w and plane_stride pitch * h, grey w whatever the layout
    it = rgb(10, 4), it.dst_pitch = 29;
    CHECK(plan1(it) == JPEGGPU_INVALID_ARGUMENT);
    it.dst_pitch = 30;
    CHECK(plan1(it) == JPEGGPU_SUCCESS);
    CHECK(plan1(it, CHW) == JPEGGPU_INVALID_ARGUMENT); // plane_stride 0
    it.dst_pitch = 10, it.plane_stride = 39;
    CHECK(plan1(it, CHW) == JPEGGPU_INVALID_ARGUMENT);
    it.plane_stride = 40;
    CHECK(plan1(it, CHW) == JPEGGPU_SUCCESS);
    it.dst_pitch = 9;
    CHECK(plan1(it, CHW) == JPEGGPU_INVALID_ARGUMENT);
    for (int layout : {HWC, CHW}) {
        it = grey(10, 4), it.dst_pitch = 9;
        CHECK(plan1(it, layout) == JPEGGPU_INVALID_ARGUMENT);
        it.dst_pitch = 10;
        CHECK(plan1(it, layout) == JPEGGPU_SUCCESS);
    }
    // the first item that fails decides, wherever it stands
    std::vector<jpeggpu_ext_roundtrip_item> items(5, rgb(9, 9));
    items[3].quality = 0;
    CHECK(plan(items, HWC, p) == JPEGGPU_INVALID_ARGUMENT);
    // a call of 2^31 blocks: 32 grey items of 65535 x 65535 are 32 * 8192^2 blocks; 31 of them are not
    items.assign(31, grey(65535, 65535));
    CHECK(plan(items, HWC, p) == JPEGGPU_SUCCESS && p.tiles == 31u * (8192u * 8192u / 256u));
    items.push_back(grey(65535, 65535));
    CHECK(plan(items, HWC, p) == JPEGGPU_NOT_SUPPORTED);
    CHECK(jpeggpu_ext_roundtrip_scratch_size(items.data(), 32) == 0);
    items[7].quality = 101; // an invalid item is refused as such, not as too large
    CHECK(plan(items, HWC, p) == JPEGGPU_INVALID_ARGUMENT);
}

void check_tiles()
{
    // grey items of exactly 1, 255, 256 and 257 blocks, in both orders: an item's first tile starts a new tile
    const int w[4] = {8, 8 * 255, 8 * 256, 8 * 257}, tiles[4] = {1, 1, 1, 2};
    for (int rev = 0; rev < 2; ++rev) {
        std::vector<jpeggpu_ext_roundtrip_item> items;
        for (int k = 0; k < 4; ++k) items.push_back(grey(w[rev ? 3 - k : k], 8));
        jg::rt::Plan p;
        CHECK(plan(items, JPEGGPU_EXT_HWC, p) == JPEGGPU_SUCCESS);
        uint32_t at = 0;
        for (int k = 0; k < 4; ++k) {
            const int j = rev ? 3 - k : k;
            CHECK(p.items[k].tile_start == at && p.items[k].blocks == w[j] / 8);
            at += tiles[j];
        }
        CHECK(p.tiles == 5 && p.n_rgb == 0 && p.off_items == 0 && p.total == p.head);
        check_fill(p);
    }
    // the same counts as RGB: 4:2:0 at 16 x 16 is 4 + 2 blocks, 136 x 120 is 17 * 15 + 2 * 9 * 8 = 399
    jg::rt::Plan p;
    CHECK(plan({rgb(16, 16), rgb(136, 120), grey(3, 3), rgb(5, 5, 50, JPEGGPU_EXT_SUBSAMPLING_444)}, JPEGGPU_EXT_HWC, p) == JPEGGPU_SUCCESS);
    CHECK(p.items[0].blocks == 6 && p.items[1].blocks == 399 && p.items[2].blocks == 1 && p.items[3].blocks == 3);
    CHECK(p.items[1].tile_start == 1 && p.items[2].tile_start == 3 && p.items[3].tile_start == 4 && p.tiles == 5 && p.n_rgb == 3);
    check_fill(p);
}

void check_layout()
{
    // planes: inside the scratch, 256-aligned, whole blocks, not overlapping; the second stage reads libjpeg's sizes
    std::vector<jpeggpu_ext_roundtrip_item> items;
    const int sizes[][2] = {{1, 1}, {2, 3}, {3, 2}, {5, 4}, {7, 5}, {8, 8}, {9, 17}, {16, 16}, {17, 33}, {33, 6}, {64, 48}, {250, 131}};
    for (const auto& s : sizes)
        for (int ss = 0; ss < 3; ++ss) {
            items.push_back(rgb(s[0], s[1], 75, ss));
            items.push_back(grey(s[0], s[1]));
        }
    size_t before = 0;
    for (size_t n = 1; n <= items.size(); ++n) { // the scratch size never shrinks as the list grows
        const size_t need = jpeggpu_ext_roundtrip_scratch_size(items.data(), static_cast<int>(n));
        CHECK(need >= before && need > 256);
        before = need;
    }
    for (int layout : {JPEGGPU_EXT_HWC, JPEGGPU_EXT_CHW}) {
        for (auto& it : items)
            if (it.channels == 3) it.dst_pitch = layout == JPEGGPU_EXT_HWC ? 3 * it.width : it.width, it.plane_stride = size_t(it.width) * it.height;
        jg::rt::Plan p;
        CHECK(plan(items, layout, p) == JPEGGPU_SUCCESS);
        CHECK(p.total + 256 == before && p.head % 256 == 0 && p.off_items == jg::rgb_batch_layout(p.n_rgb).total);
        CHECK(p.rgb.jobs.size() == size_t(p.n_rgb) && p.rgb.t_tiles == 0 && !p.rgb.all_models);
        size_t at = p.head;
        int k     = 0;
        for (size_t i = 0; i < items.size(); ++i) {
            const jg::rt::Item& it = p.items[i];
            if (it.channels == 1) {
                CHECK(it.dst == kDst && it.pitch[0] == items[i].dst_pitch);
                continue;
            }
            for (int c = 0; c < 3; ++c) {
                const int bw = c ? it.mcus_x : it.grid_w, bh = c ? it.mcus_y : it.grid_h, pitch = it.pitch[c > 0];
                CHECK(it.plane_off[c] == at && at % 256 == 0 && pitch % 16 == 0 && pitch >= 8 * bw);
                at += (size_t(pitch) * 8 * bh + 255) / 256 * 256;
                const jg::FancyComp& f = p.rgb.jobs[k].src.comp[c];
                CHECK(f.plane == kBase + it.plane_off[c] && f.pitch == pitch && f.w <= 8 * bw && f.h <= 8 * bh);
                CHECK(f.w == (c ? (it.width + it.hs - 1) / it.hs : it.width) && f.h == (c ? (it.height + it.vs - 1) / it.vs : it.height));
                CHECK(f.hr == (c ? it.hs : 1) && f.vr == (c ? it.vs : 1));
                CHECK(f.mode == jg::fancy_mode(f.hr, f.vr, f.w)); // replication where the downsampled width is at most 2
            }
            CHECK(p.rgb.jobs[k].width == it.width && p.rgb.jobs[k].height == it.height && p.rgb.jobs[k].dst == kDst);
            ++k;
        }
        CHECK(at == p.total && k == p.n_rgb);
        check_fill(p);
    }
}

} // namespace

int main(int argc, char** argv)
{
    if (argc > 1) {
        if ((argc - 1) % 5 != 0) return 2;
        for (int a = 1; a < argc; a += 5) {
            jpeggpu_ext_roundtrip_item s = rgb(std::atoi(argv[a]), std::atoi(argv[a + 1]), std::atoi(argv[a + 4]), std::atoi(argv[a + 3]));
            s.channels                   = std::atoi(argv[a + 2]);
            if (plan1(s.channels == 1 ? grey(s.width, s.height, s.quality) : s) != JPEGGPU_SUCCESS) return 3;
            jg::rt::Item it;
            jg::rt::item_geometry(s, it);
            std::printf("%d %d %d %d %d %d %d |", it.hs, it.vs, it.mcus_x, it.mcus_y, it.grid_w, it.grid_h, it.blocks);
            for (int t = 0; t < 2; ++t) {
                for (int i = 0; i < 64; ++i) std::printf(" %d", it.quant[t][i]);
                std::printf(t ? "\n" : " |");
            }
        }
        return 0;
    }
    check_refusals();
    check_tiles();
    check_layout();
    std::printf("roundtrip plan check: %d checks passed\n", g_checks);
    return 0;
}

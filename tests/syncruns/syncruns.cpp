// syncruns.cpp -- host model of the batched sequence kernel with RUNS of subsequences per lane (jg_sync_runs.h), for CPU
// tests: the product's own lane functions (run_plan / run_speculate / run_flow), called one lane at a time over the
// groups of a whole scan, on the product's parse and sync pack. Compiled with g++ from the product's sources the way
// tests/syncprobe is.
//
// Three things here are restatements and not the product's code:
//   * the sequential decoder: every subsequence from its predecessor's true exit state, segment by segment -- the truth;
//   * the tail's rule (huff_sync_tail): a flow from every marked entry and every sequence boundary inside a segment,
//     in stream order, until the state it reaches is the stored one;
//   * today's schedule of one subsequence per lane (huff_sync_intra_batch's R = 1 body), which the R = 1 table and marks of
//     the shared lane functions must equal.
#include "jg_sync_runs.h"
#include "jg_reader.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

using namespace jg;

namespace {

struct Table { // what the kernels keep per subsequence
    std::vector<int> p, n, cz;
    std::vector<uint32_t> dc01, dc23;
    std::vector<uint8_t> pending;
    explicit Table(int S) : p(S, -1), n(S, -1), cz(S, -1), dc01(S, 0xDEADu), dc23(S, 0xDEADu), pending(S, 0xEE) {}
    void put(int sub, const LaneState& st, int czv, bool pend)
    {
        p[sub] = st.p, n[sub] = st.n, cz[sub] = czv, dc01[sub] = st.dc01, dc23[sub] = st.dc23;
        pending[sub] = pend ? 1 : 0;
    }
    bool same_entry(const Table& o, int i) const { return p[i] == o.p[i] && n[i] == o.n[i] && cz[i] == o.cz[i] && dc01[i] == o.dc01[i] && dc23[i] == o.dc23[i]; }
};

struct ScanData {
    std::vector<uint8_t> dst; // destuffed, linear: subsequence s at s * subseq_bytes
    std::vector<Segment> segments;
    std::vector<int> seg_idx;
    std::vector<uint8_t> tabs;
    ScanParams sp{};
    int S = 0, subseq_bytes = 0;
};

struct HostFetch { // the bytes of the segment the row lies in, linear; zero outside (as tests/syncprobe)
    const ScanData* sd;
    const uint8_t* seg;
    int seg_words;
    typedef int Pos;
    void set_row(int sub, int rel)
    {
        seg       = sd->dst.data() + static_cast<size_t>(sub - rel) * sd->subseq_bytes;
        seg_words = sd->segments[sd->seg_idx[sub]].subseq_count * (sd->subseq_bytes / 4);
    }
    Pos start(int w) const { return w; }
    void advance(Pos& q) const { ++q; }
    uint32_t load(const Pos& w) const
    {
        if (w < 0 || w >= seg_words) return 0;
        const uint8_t* p = seg + static_cast<size_t>(w) * 4;
        return static_cast<uint32_t>(p[0]) << 24 | p[1] << 16 | p[2] << 8 | p[3];
    }
    uint32_t cook(uint32_t v, const Pos&) const { return v; }
};

struct HostIo {
    const ScanData* sd;
    Table* tab;
    int e1_p[kSeqLanes + 1], e1_cz[kSeqLanes + 1];
    long long spec = 0, flow = 0;
    Segment segment_of(int sub) const { return sd->segments[sd->seg_idx[sub]]; }
    void put_e1(int lane, int p, int cz)
    {
        e1_p[lane] = p, e1_cz[lane] = cz;
        ++spec;
    }
    bool e1_is(int lane, int p, int cz) const { return e1_p[lane] == p && e1_cz[lane] == cz; }
    void store(int sub, const LaneState& st, int cz, bool pending)
    {
        tab->put(sub, st, cz, pending);
        ++flow;
    }
};

void destuff(const uint8_t* bytes, const Scan& sc, int subseq_bytes, std::vector<uint8_t>& dst)
{
    dst.assign(static_cast<size_t>(sc.num_subseq) * subseq_bytes + 256, 0);
    for (const DestuffChunk& ck : sc.chunks) {
        uint32_t o = ck.dst_off;
        for (uint32_t pos = ck.begin; pos < ck.end; ++pos) {
            uint32_t p = pos > 0 ? bytes[pos - 1] : 0;
            if (ck.first && pos == ck.begin) p = 0;
            const uint32_t b = bytes[pos];
            if (p == 0xFF && b == 0) dst[o++] = 0xFF;
            else if (p != 0xFF && b != 0xFF) dst[o++] = static_cast<uint8_t>(b);
        }
    }
}

/// One state-only decode of subsequence `sub` (index `rel` in its segment) from (p, c, z), sums from zero.
template <class Sink>
void decode_one(const ScanData& sd, int sub, int rel, LaneState& st)
{
    HostFetch f{&sd, nullptr, 0};
    f.set_row(sub, rel);
    st.n = 0, st.dc01 = 0, st.dc23 = 0;
    BitWindow<HostFetch> bw{};
    bw.seek(st.p, f);
    Sink sink;
    decode_subsequence(st, bw, f, (rel + 1) * sd.subseq_bytes * 8, sd.tabs.data(), sd.sp, sink);
}

void sequential(const ScanData& sd, Table& t)
{
    for (const Segment& seg : sd.segments) {
        LaneState st{};
        for (int rel = 0; rel < seg.subseq_count; ++rel) {
            decode_one<NoSink>(sd, seg.subseq_offset + rel, rel, st);
            t.put(seg.subseq_offset + rel, st, st.c | (st.z << 8), false);
        }
    }
}

/// The schedule of one subsequence per lane, restated from huff_sync_intra_batch's R = 1 body (one flow iteration).
void todays_schedule(const ScanData& sd, Table& t)
{
    const int SEQ = kSeqSubseqBatch, T = kSeqLanes, OV = T - SEQ, S = sd.S;
    for (int seq = 0; seq * SEQ < S; ++seq) {
        const int img_first = seq * SEQ - OV, img_end = std::min(T, S - img_first);
        std::vector<LaneState> e1(T);
        for (int l = 0; l < img_end; ++l) {
            const int sub = img_first + l;
            if (sub < 0) continue;
            const Segment seg = sd.segments[sd.seg_idx[sub]];
            e1[l]   = LaneState{};
            e1[l].p = (sub - seg.subseq_offset) * sd.subseq_bytes * 8;
            decode_one<SpecSink>(sd, sub, sub - seg.subseq_offset, e1[l]);
        }
        for (int l = 0; l + 1 < img_end; ++l) {
            const int j = img_first + l + 1; // the entry this lane's flow decodes
            if (j < 0) continue;
            const Segment seg = sd.segments[sd.seg_idx[j]];
            const bool opens  = j == seg.subseq_offset;
            LaneState st      = opens ? LaneState{} : e1[l];
            decode_one<NoSink>(sd, j, j - seg.subseq_offset, st);
            const int cz      = st.c | (st.z << 8);
            const bool synced = st.p == e1[l + 1].p && cz == (e1[l + 1].c | (e1[l + 1].z << 8));
            const int lim     = std::min(img_end, seg.subseq_offset + seg.subseq_count - img_first);
            t.put(j, st, cz, !synced && l + 2 < lim);
        }
    }
}

/// The tail's rule. Returns the decodes it took.
long long tail_rule(const ScanData& sd, Table& t)
{
    const int SEQ = sd.sp.seq_subseq, S = sd.S;
    long long decodes = 0;
    for (int from = 0; from + 1 < S; ++from) {
        bool f = t.pending[from] != 0;
        if (!f && (from + 1) % SEQ == 0 && sd.seg_idx[from] == sd.seg_idx[from + 1]) f = true; // bnd_p == -1: every boundary
        if (!f) continue;
        LaneState st{};
        st.p = t.p[from], st.c = t.cz[from] & 0xFF, st.z = t.cz[from] >> 8;
        for (int j = from + 1;; ++j) {
            const Segment seg = sd.segments[sd.seg_idx[j - 1]];
            const int lim     = seg.subseq_offset + seg.subseq_count;
            if (j >= lim) break;
            decode_one<NoSink>(sd, j, j - seg.subseq_offset, st);
            ++decodes;
            const int cz       = st.c | (st.z << 8);
            const bool flowing = !(st.p == t.p[j] && cz == t.cz[j]) && j + 1 < lim;
            t.put(j, st, cz, t.pending[j] != 0);
            if (!flowing) break;
        }
    }
    return decodes;
}

template <int W, int R>
void run_schedule(const ScanData& sd, Table& t, HostIo& io)
{
    const int SEQ = sd.sp.seq_subseq, S = sd.S;
    for (int g0 = 0; g0 < S; g0 += SEQ * R) {
        std::vector<RunLane> lanes(kSeqLanes);
        HostFetch f{&sd, nullptr, 0};
        for (int l = 0; l < kSeqLanes; ++l) {
            run_plan<R>(lanes[l], l, g0, SEQ, S);
            const Segment seg = lanes[l].active ? io.segment_of(lanes[l].a) : Segment{0, 0};
            run_speculate<W>(lanes[l], l, seg, f, sd.tabs.data(), sd.sp, io);
        }
        // (the barrier: every E1 of the group is there)
        for (int l = 0; l < kSeqLanes; ++l) run_flow<W, R>(lanes[l], l, f, sd.tabs.data(), sd.sp, io);
    }
    (void)t;
}

template <int W>
bool run_schedule_r(int R, const ScanData& sd, Table& t, HostIo& io)
{
    switch (R) {
    case 1: run_schedule<W, 1>(sd, t, io); return true;
    case 2: run_schedule<W, 2>(sd, t, io); return true;
    case 4: run_schedule<W, 4>(sd, t, io); return true;
    }
    return false;
}

} // namespace

extern "C" {

/// The run schedule with R subsequences per lane over scan `scan` of a file at `subseq_bytes` (128 or 256).
/// out[0] subsequences; [1] groups; [2] speculative decodes; [3] flow decodes; [4] entries whose stored (p, cz) is not the
/// sequential decoder's, before the tail's rule; [5] marks; [6] marks that are not at a run start; [7] entries of which
/// any of the five words differs from the sequential decoder's AFTER the tail's rule; [8] entries whose words or mark
/// differ from today's schedule (R == 1 only, else -1); [9] decodes of the tail's rule; [10] entries the schedule
/// never stored; [11] restart segments; [12 + k] segments that open at a subsequence index with index % 4 == k;
/// [16 + k] segments of k subsequences (k = 1 .. 7; [16]: of more). Returns a jpeggpu_status, or -1 for parameters the probe does not take.
int probe_sync_runs(const uint8_t* data, size_t size, int subseq_bytes, int scan, int R, long long* out)
{
    Reader rd;
    Logger log;
    const jpeggpu_status stat = rd.parse(data, size, subseq_bytes, log);
    if (stat != JPEGGPU_SUCCESS) return stat;
    const Stream& s = rd.s;
    if (scan < 0 || scan >= s.num_scans) return -1;
    const Scan& sc = s.scans[scan];
    std::vector<uint8_t> bytes(s.xfer_end - s.xfer_begin + 2 * kDestuffWin, 0);
    std::memcpy(bytes.data(), data + s.xfer_begin, s.xfer_end - s.xfer_begin);

    ScanData sd;
    sd.S = sc.num_subseq, sd.subseq_bytes = subseq_bytes;
    destuff(bytes.data(), sc, subseq_bytes, sd.dst);
    sd.segments.assign(sc.segments.begin(), sc.segments.end());
    sd.seg_idx.assign(static_cast<size_t>(sd.S), 0);
    for (size_t g = 0; g < sd.segments.size(); ++g)
        for (int k = 0; k < sd.segments[g].subseq_count; ++k) sd.seg_idx[static_cast<size_t>(sd.segments[g].subseq_offset + k)] = static_cast<int>(g);
    sd.tabs               = sc.table_pack_sync;
    sd.sp.du_per_mcu      = sc.du_per_mcu;
    sd.sp.num_comp        = sc.num_comp;
    sd.sp.subseq_words    = subseq_bytes / 4;
    sd.sp.num_subseq      = sd.S;
    sd.sp.seq_subseq      = kSeqSubseqBatch;
    sd.sp.tab_bytes_sync  = static_cast<uint32_t>(sc.table_pack_sync.size());
    sd.sp.cursor_off_sync = sc.cursor_off_sync;
    sd.sp.use_sync_pack();

    const int S = sd.S;
    Table truth(S), got(S);
    sequential(sd, truth);
    HostIo io{&sd, &got, {}, {}};
    const bool ok = subseq_bytes == 128 ? run_schedule_r<32>(R, sd, got, io) : subseq_bytes == 256 ? run_schedule_r<64>(R, sd, got, io) : false;
    if (!ok) return -1;

    long long wrong = 0, marks = 0, marks_inside = 0, never = 0, vs_today = -1;
    for (int i = 0; i < S; ++i) {
        never += got.pending[i] == 0xEE;
        wrong += got.p[i] != truth.p[i] || got.cz[i] != truth.cz[i];
        marks += got.pending[i] == 1;
        marks_inside += got.pending[i] == 1 && i % R != 0;
    }
    if (R == 1) {
        Table today(S);
        todays_schedule(sd, today);
        vs_today = 0;
        for (int i = 0; i < S; ++i) vs_today += !got.same_entry(today, i) || got.pending[i] != today.pending[i];
    }
    const long long tail = never == 0 ? tail_rule(sd, got) : 0;
    long long bad = 0;
    for (int i = 0; i < S; ++i) bad += !got.same_entry(truth, i);
    out[0] = S, out[1] = (S + kSeqSubseqBatch * R - 1) / (kSeqSubseqBatch * R), out[2] = io.spec, out[3] = io.flow;
    out[4] = wrong, out[5] = marks, out[6] = marks_inside, out[7] = bad, out[8] = vs_today, out[9] = tail, out[10] = never;
    out[11] = static_cast<long long>(sd.segments.size());
    for (int k = 12; k < 24; ++k) out[k] = 0;
    for (const Segment& seg : sd.segments) {
        if (seg.subseq_count == 0) continue;
        ++out[12 + seg.subseq_offset % 4];
        ++out[16 + (seg.subseq_count <= 7 ? seg.subseq_count : 0)];
    }
    return JPEGGPU_SUCCESS;
}

/// Subsequences of scan `scan` of a file at `subseq_bytes` (negative: the parse failed or there is no such scan).
int probe_num_subseq(const uint8_t* data, size_t size, int subseq_bytes, int scan)
{
    Reader rd;
    Logger log;
    if (rd.parse(data, size, subseq_bytes, log) != JPEGGPU_SUCCESS || scan < 0 || scan >= rd.s.num_scans) return -1;
    return rd.s.scans[scan].num_subseq;
}

} // extern "C"

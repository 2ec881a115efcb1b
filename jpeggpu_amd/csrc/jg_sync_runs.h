// jg_sync_runs.h -- the schedule of ONE LANE of the batched sequence kernel when a lane owns a RUN of consecutive
// subsequences (huff_sync_intra_batch<W, JS, R>, R > 1), shared by the kernel and by a host twin that calls it one lane at
// a time (tests/syncruns), the way decode_subsequence is shared.
//
// With one subsequence per lane every byte of a scan is decoded twice, state-only: once from the guessed state
// (c, z) = (0, 0) to learn an exit state, once from the exit state of the lane in front to get n and the DC sums. The
// first decode only makes a start state for the second, and a flow that is already running needs none: its start state
// is the state it has. A lane that owns the run [a, a + r), r <= R, therefore
//   1. speculates subsequence a from (0, 0): its exit state E1(a) (exact where a opens a restart segment);
//   2. flows through a + 1 .. a + r - 1 from the state it is in and stores their entries, not marked;
//   3. flows on into a + r, the first subsequence of the next lane's run, stores that entry, and marks it `pending`
//      iff the state it leaves a + r in is not the E1(a + r) the next lane went on from (and a flow could go on there):
// R + 1 decodes per R subsequences instead of 2 R. A subsequence that opens a restart segment is decoded from the
// segment's start state wherever in a run it lies. Marks can only appear at run starts; the states inside a run come from
// one flow, so the entry behind a stored state was decoded from that very state, which is all huff_sync_tail asks of
// entries that carry no mark (its CONTRACT, jg_kernels.hip).
//
// The lanes of a group: lane 0 is the overlap lane, whose "run" is the one subsequence in front of the group -- it
// speculates that, flows into the group's first subsequence and owns nothing; lanes 1 .. `seq` own runs of R; the last
// of them does not flow out (the next group's overlap lane does). E1 goes from lane to lane through `Io` (LDS on the
// device, two ints per lane) with ONE barrier between run_speculate and run_flow; everything else goes from registers
// to the state arrays.
//
//   Fetch: what BitWindow asks (jg_huff_core.h) plus set_row(sub, rel): work in the row of subsequence `sub` of the scan,
//          which is subsequence `rel` of its segment.
//   Io:    Segment segment_of(int sub)                      the restart segment subsequence `sub` lies in
//          void put_e1(int lane, int p, int cz)             publish the lane's speculated exit state
//          bool e1_is(int lane, int p, int cz)              is that what `lane` published?
//          void store(int sub, const LaneState&, int cz, bool pending)   the five state words and the mark of an entry
#ifndef JG_SYNC_RUNS_H_
#define JG_SYNC_RUNS_H_

#include "jg_huff_core.h"

namespace jg {

struct RunLane {
    int a;       // first subsequence of the run (the overlap lane: the subsequence in front of the group)
    int next;    // first subsequence of the next lane's run, which this lane flows out into (-1: it does not)
    int last;    // last subsequence the lane decodes as a flow (below a + 1: none)
    int end;     // one past the group's last subsequence
    bool active; // subsequence a exists: the lane speculates
    Segment seg; // restart segment of the subsequence decoded last ...
    int rel;     // ... and that subsequence's index in it
    LaneState st;
};

/// The run of lane `l` of the group whose first subsequence is `g0`; `seq` lanes behind the overlap lane own runs
/// (ScanParams::seq_subseq), `S` subsequences in the scan.
template <int R>
JG_HD inline void run_plan(RunLane& ln, int l, int g0, int seq, int S)
{
    const bool overlap = l == 0;
    ln.a               = overlap ? g0 - 1 : g0 + (l - 1) * R;
    ln.active          = ln.a >= 0 && ln.a < S && l <= seq;
    ln.next            = l < seq ? (overlap ? g0 : ln.a + R) : -1;
    ln.last            = l > seq ? ln.a : l == seq ? ln.a + R - 1 : ln.next;
    if (ln.last > S - 1) ln.last = S - 1;
    ln.end = g0 + seq * R < S ? g0 + seq * R : S;
    // (a lane without a subsequence of its own -- the overlap lane of the scan's first group -- stands "at the end of
    // a segment": its flow opens the next one, from the segment's start state)
    ln.seg = Segment{0, 0};
    ln.rel = -1;
    ln.st  = LaneState{};
}

/// Step 1: the lane's own first subsequence from the guessed state, exit state only. `seg`: the segment it lies in.
template <int W, class Fetch, class Io>
JG_HD inline void run_speculate(RunLane& ln, int l, const Segment& seg, Fetch& fetch, const uint8_t* tabs, const ScanParams& sp, Io& io)
{
    constexpr int kBits = W * 32;
    if (!ln.active) return;
    ln.seg  = seg;
    ln.rel  = ln.a - seg.subseq_offset;
    ln.st.p = ln.rel * kBits;
    fetch.set_row(ln.a, ln.rel);
    BitWindow<Fetch> bw{};
    bw.seek(ln.st.p, fetch);
    SpecSink none;
    decode_subsequence(ln.st, bw, fetch, (ln.rel + 1) * kBits, tabs, sp, none);
    io.put_e1(l, ln.st.p, ln.st.c | (ln.st.z << 8));
}

/// Steps 2 and 3, behind the barrier that makes every lane's E1 visible: ONE loop with one copy of the symbol loop.
template <int W, int R, class Fetch, class Io>
JG_HD inline void run_flow(RunLane& ln, int l, Fetch& fetch, const uint8_t* tabs, const ScanParams& sp, Io& io)
{
    constexpr int kBits = W * 32;
    NoSink sink;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma nounroll
#endif
    for (int k = 1; k <= R; ++k) {
        const int j = ln.a + k;
        if (j > ln.last) break;
        if (ln.rel + 1 == ln.seg.subseq_count) { // j opens the next segment: from its start state, which is known
            ln.seg = io.segment_of(j);
            ln.rel = -1;
            ln.st  = LaneState{};
        }
        ln.st.n    = 0;
        ln.st.dc01 = 0;
        ln.st.dc23 = 0;
        // every decode works in the row of its subsequence: the window is set up again from p
        ++ln.rel;
        fetch.set_row(j, ln.rel);
        BitWindow<Fetch> bw{};
        bw.seek(ln.st.p, fetch);
        decode_subsequence(ln.st, bw, fetch, (ln.rel + 1) * kBits, tabs, sp, sink);
        const int cz = ln.st.c | (ln.st.z << 8);
        // the next lane went on from its E1(j): if that is not where this flow leaves j, the flow is cut short here and
        // huff_sync_tail continues it -- unless nothing follows j in its segment or in the group (the group's last entry
        // is a sequence boundary, where the tail kernel starts a flow anyway)
        bool pending = false;
        if (j == ln.next) pending = !io.e1_is(l + 1, ln.st.p, cz) && j + 1 < ln.end && ln.rel + 1 < ln.seg.subseq_count;
        io.store(j, ln.st, cz, pending);
    }
}

} // namespace jg

#endif // JG_SYNC_RUNS_H_

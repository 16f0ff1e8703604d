// The step schedule of the fused dense-block kernel (rdb_f16x2.hip, rdb_f16x2_kernel) and its proof: which barrier an
// MFMA wave takes where, what the DMA waves issue in which interval and how much of it a barrier's counted wait may
// leave in flight -- and a compile-time walk over the 40 steps showing that no ring position is refilled while it is
// read, or read before the wait that covers it.  The kernel's loops call the functions the walk calls.  Plain constexpr
// C++ (no HIP header, no device qualifier): a host compiler checks the asserts on this file alone.
#pragma once

namespace nesr {

constexpr int RDB_STEP5 = 4 + 6 + 8 + 10;     // conv5's first step: its steps take two weight slabs each (all 64 output channels)
constexpr int RDB_STEPS = RDB_STEP5 + 12;     // K-chunk steps of a dense block

// The stagger.  MFMA waves w and w + 4 share a SIMD and run the same program: with one barrier on top of every step both
// reach the address updates, the fragment waits, the barrier and the ramp behind it together, and the matrix pipe has
// nothing to issue meanwhile.  NESR_RDB_LAG = L > 0 delays waves 4..7 by L tap-steps inside each of conv1..conv4: they take
// the barrier of step s + 1 in front of tap-step 5 - L of step s, so between two barriers they run the last L tap-steps of
// one step and the first 5 - L of the next, and their step boundary falls into the middle of their partner's MFMAs.
// Per layer they re-converge: a layer's first step has the barrier on top as well (the deferred epilogue runs there in
// both partners at once), its last step has none.  conv5 runs aligned.
#ifndef NESR_RDB_LAG
#define NESR_RDB_LAG 2
#endif
namespace rdbs {
constexpr int LAG = NESR_RDB_LAG;
static_assert(LAG == 2 || LAG == 3, "NESR_RDB_LAG: 2 (barrier in front of tap-step 3) or 3 (in front of tap-step 2)");
constexpr int layer_of(int s) { return s < 4 ? 0 : s < 10 ? 1 : s < 18 ? 2 : s < RDB_STEP5 ? 3 : 4; }
constexpr int first_of(int l) { return l == 0 ? 0 : l == 1 ? 4 : l == 2 ? 10 : l == 3 ? 18 : RDB_STEP5; }
constexpr int steps_of(int l) { return l == 4 ? RDB_STEPS - RDB_STEP5 : 4 + 2 * l; }
// ---- MFMA role: where a step's barriers sit and when its first fragments are requested
enum Mode {
    M_LEAD,         // waves 0..3: barrier on top; the step's first fragments are requested behind it
    M_LAG_FIRST,    // waves 4..7, a layer's first step: as M_LEAD, and the next barrier in front of tap-step 5 - LAG
    M_LAG_MID,      // waves 4..7: one barrier, in front of tap-step 5 - LAG
    M_LAG_LAST,     // waves 4..7, a layer's last step: no barrier, no request for the next step
    M_CONV5         // barrier on top; weights behind it, the next step's first pixel fragments beside tap-step 4
};
constexpr int mode_of(bool lagging, int s) {
    const int l = layer_of(s), c = s - first_of(l);
    return l == 4 ? M_CONV5 : !lagging ? M_LEAD : c == 0 ? M_LAG_FIRST : c == steps_of(l) - 1 ? M_LAG_LAST : M_LAG_MID;
}
constexpr bool bar_top(int m) { return m != M_LAG_MID && m != M_LAG_LAST; }
constexpr int bar_tap(int m) { return m == M_LAG_FIRST || m == M_LAG_MID ? 5 - LAG : -1; }      // the barrier in front of this tap-step
constexpr bool req_behind(int m) { return m == M_LEAD || m == M_LAG_FIRST; }                    // tap-step 0's fragments: behind the top barrier
constexpr bool req_early(int m) { return m == M_LAG_FIRST || m == M_LAG_MID; }    // the next step's: beside tap-step 4
// ---- DMA role.  Input chunk and weight slab of step t go to ring position t & 3 (conv5's slab pair: 0,1 / 2,3).
// Waves 4..7 still read step s - 1 behind barrier s, so conv1..conv4 are
// fetched TWO steps ahead (interval s = barrier s .. barrier s + 1 issues step s + 2 into the position of step s - 2);
// conv5 needs three again (its pixel prefetch crosses the barrier): the catch-up chunk goes out in conv5's first
// interval, when waves 4..7 have left conv4's last two slots.
constexpr int in_end(int i) {      // input steps [0, in_end(i)) are issued by the end of interval i (-1: the prologue)
    const int e = i < RDB_STEP5 ? i + 3 : i + 4;
    return e < RDB_STEPS ? e : RDB_STEPS;
}
constexpr int IN_LEAD = in_end(-1);
constexpr bool w_slab(int i) { return i + 1 < RDB_STEP5 && in_end(i - 1) < RDB_STEP5; }      // interval i issues a conv1..conv4 slab (that of its input step)
constexpr bool w_pair(int i) { return i + 1 >= RDB_STEP5 && i + 1 < RDB_STEPS; }             // interval i issues conv5's slab pair of step i + 1
// Issue order inside an interval: weights, then the input chunks in step order -- the order the next barrier needs them
// in.  These many of the interval's LAST issues may still be in flight at the next barrier (counted wait):
constexpr int tail_w(int i) { return w_slab(i) ? 1 : 0;}
constexpr int tail_in(int i) {
    const int n = in_end(i) - in_end(i - 1);
    return i == RDB_STEP5 - 1 ? 0       // conv5's first step prefetches step 29's pixels: nothing stays in flight
         : i == RDB_STEP5 ? 1           // the catch-up: step 30 has landed at barrier 29, step 31 need not
         : n;
}
// ---- the proof: a walk over the 40 steps with the functions above (the kernel's loops use the same ones)
struct Walk {
    int in_iss[RDB_STEPS] = {}, w_iss[RDB_STEPS] = {};          // interval that issues step t's input chunk / weights (-2: the prologue)
    int in_land[RDB_STEPS] = {}, w_land[RDB_STEPS] = {};        // barrier (-1: the one in front of step 0's) whose wait covers them
    int rd_lo[2][RDB_STEPS + 1] = {}, rd_hi[2][RDB_STEPS + 1] = {};   // [waves 0..3 | 4..7][interval + 1]: steps whose slots are read (input)
    int wr_hi[2][RDB_STEPS + 1] = {};                                 // the same for weights (the lower end is rd_lo)
    int bars[3] = {};                                           // s_barrier count: waves 0..3, waves 4..7, DMA waves
    bool ok = true;
};
constexpr bool pos_overlap_w(int t, int u) {      // do the weights of steps t and u share a ring slab?
    const int t0 = t < RDB_STEP5 ? (t & 3) : (t & 1) * 2, t1 = t < RDB_STEP5 ? t0 : t0 + 1;
    const int u0 = u < RDB_STEP5 ? (u & 3) : (u & 1) * 2, u1 = u < RDB_STEP5 ? u0 : u0 + 1;
    return t0 <= u1 && u0 <= t1;
}
constexpr Walk walk() {
    Walk k;
    // MFMA roles: which interval every tap-step (and every fragment request) falls into
    for (int r = 0; r < 2; ++r) {
        for (int i = 0; i <= RDB_STEPS; ++i) { k.rd_lo[r][i] = RDB_STEPS; k.rd_hi[r][i] = -1; k.wr_hi[r][i] = -1; }
        int b = 1;      // barriers taken so far (the extra one in front of step 0's is the first): the wave is in interval b - 2
        auto rd = [&](int t, bool pix, bool wts) {
            if (t < k.rd_lo[r][b - 1]) k.rd_lo[r][b - 1] = t;
            if (pix && t > k.rd_hi[r][b - 1]) k.rd_hi[r][b - 1] = t;
            if (wts && t > k.wr_hi[r][b - 1]) k.wr_hi[r][b - 1] = t;
        };
        for (int s = 0; s < RDB_STEPS; ++s) {
            const int m = mode_of(r, s);
            if (bar_top(m)) ++b;
            for (int t = 0; t < 5; ++t) {
                if (t == bar_tap(m)) ++b;
                rd(s, true, true);
                // the request for the next step
                if (t == 4 && req_early(m)) rd(s + 1, true, s + 1 < RDB_STEP5);
                if (t == 4 && m == M_CONV5 && s + 1 < RDB_STEPS) rd(s + 1, true, false);
            }
        }
        k.bars[r] = b;
    }
    // DMA role: the issue queue in order (vmcnt retires in order), and what every barrier's counted wait leaves in flight
    int q_step[3 * RDB_STEPS] = {}, q_w[3 * RDB_STEPS] = {}, qn = 0, landed = 0;
    auto land = [&](int upto, int b) {
        for (; landed < upto; ++landed) (q_w[landed] ? k.w_land : k.in_land)[q_step[landed]] = b;
    };
    for (int t = 0; t < IN_LEAD; ++t) {
        q_step[qn] = t; q_w[qn++] = 1; k.w_iss[t] = -2;
        q_step[qn] = t; q_w[qn++] = 0; k.in_iss[t] = -2;
    }
    land(qn - 2 * (IN_LEAD - 1), -1);
    int tail = 2;      // barrier 0: one step of the prologue may still be in flight
    k.bars[2] = 1;
    for (int i = 0; i < RDB_STEPS; ++i) {
        land(qn - tail, i);
        ++k.bars[2];
        const int f = in_end(i - 1), e = in_end(i);
        if (w_pair(i)) { q_step[qn] = i + 1; q_w[qn++] = 1; k.w_iss[i + 1] = i; }
        else if (w_slab(i)) {
            if (e - f != 1) k.ok = false;
            q_step[qn] = f; q_w[qn++] = 1; k.w_iss[f] = i;
        }
        for (int t = f; t < e; ++t) { q_step[qn] = t; q_w[qn++] = 0; k.in_iss[t] = i; }
        tail = tail_w(i) + tail_in(i);
        if (tail_w(i) && tail_in(i) != e - f) k.ok = false;      // weights are issued first: in flight only with all that follows
    }
    if (qn != 2 * RDB_STEPS) k.ok = false;
    land(qn, RDB_STEPS);
    // every read: landed at or before the barrier that opens its interval, and nothing newer issued into its position by
    // the end of that interval (= the position is no DMA destination while it is read)
    for (int r = 0; r < 2; ++r)
        for (int i = -1; i < RDB_STEPS; ++i) {
            for (int t = k.rd_lo[r][i + 1]; t <= k.rd_hi[r][i + 1]; ++t) {
                if (k.in_land[t] > i) k.ok = false;
                for (int u = t + 1; u < RDB_STEPS; ++u) if ((u & 3) == (t & 3) && k.in_iss[u] <= i) k.ok = false;
            }
            for (int t = k.rd_lo[r][i + 1]; t <= k.wr_hi[r][i + 1]; ++t) {
                if (k.w_land[t] > i) k.ok = false;
                for (int u = t + 1; u < RDB_STEPS; ++u) if (pos_overlap_w(t, u) && k.w_iss[u] <= i) k.ok = false;
            }
        }
    return k;
}
constexpr Walk WALK = walk();
static_assert(WALK.ok, "a ring position is refilled while it is read, or read before the wait that covers it");
static_assert(WALK.bars[0] == RDB_STEPS + 1 && WALK.bars[1] == RDB_STEPS + 1 && WALK.bars[2] == RDB_STEPS + 1, "every role takes the same number of barriers");

// ---- Chained blocks (rdb_f16x2_chain_kernel): the walk above runs once per block.  Behind a block's walk every role takes
// one more barrier, E (behind the final epilogue), and the DMA waves then issue the next block's first IN_LEAD steps
// in the order w[0..IN_LEAD), in[0..IN_LEAD) -- the weights in front of the poll for the previous block's `out`.
constexpr int CHAIN_BARS = RDB_STEPS + 2;       // per block and role: the one in front of step 0's, one per step, E
constexpr int REENTRY_TAIL_FIRST = IN_LEAD - 1; // input chunks that may be in flight at the next block's first barrier
constexpr int REENTRY_TAIL_0 = IN_LEAD - 2;     // ... and at its barrier 0 (no weight slab in either: they were issued first)
constexpr bool chain_reentry_ok() {
    bool ok = true;
    // nothing is issued into a slot or slab that a lagging wave of the previous block can still read: every read of the
    // walk lies in an interval in front of E (the walk has no interval past RDB_STEPS - 1), every issue of the walk has
    // landed by its last barrier, and the re-entry issues come behind E
    for (int t = 0; t < RDB_STEPS; ++t)
        if (WALK.in_land[t] > RDB_STEPS - 1 || WALK.w_land[t] > RDB_STEPS - 1) ok = false;
    // the rings are back where a block starts: step t uses position t & 3, conv5's pairs 0,1 / 2,3 alternate
    if (RDB_STEPS % 4 != 0 || RDB_STEP5 % 4 != 0 || (RDB_STEPS - RDB_STEP5) % 2 != 0) ok = false;
    // the re-entry queue w0 .. w(L-1), in0 .. in(L-1): what the first two counted waits cover against what is read behind them
    const int landed_first = IN_LEAD - REENTRY_TAIL_FIRST;      // input steps [0, landed_first) at the first barrier, every slab
    const int landed_0 = IN_LEAD - REENTRY_TAIL_0;              // ... at barrier 0
    for (int r = 0; r < 2; ++r) {
        if (WALK.rd_hi[r][0] >= landed_first || WALK.wr_hi[r][0] >= IN_LEAD) ok = false;
        if (WALK.rd_hi[r][1] >= landed_0 || WALK.wr_hi[r][1] >= IN_LEAD) ok = false;
    }
    // from interval 0 on the walk's own issues follow and its waits count them alone: barrier 1's leaves at most the
    // issues of interval 0 in flight, so the whole re-entry queue has landed there (vmcnt retires in order)
    if (tail_w(0) + tail_in(0) > 1 + (in_end(0) - in_end(-1))) ok = false;
    if (WALK.bars[0] + 1 != CHAIN_BARS || WALK.bars[1] + 1 != CHAIN_BARS || WALK.bars[2] + 1 != CHAIN_BARS) ok = false;
    return ok;
}
static_assert(chain_reentry_ok(), "re-entry at a block boundary: a ring position is refilled while a wave of the previous block can read it, read before it has landed, or the roles' barrier counts differ");

// Buffer reuse.  Dense block r (0..2) of an RRDB runs in buffer cur(r), writes x1..x4 into it and conv5's result into the
// x0 slice of out(r); its third block reads the RRDB's input from the x0 slice of res2(r) and lands there in place.
constexpr int rdb_cur_buf(int r) { return r; }
constexpr int rdb_out_buf(int r) { return r < 2 ? r + 1 : 0; }
constexpr int rdb_res2_buf(int r) { return r < 2 ? -1 : 0; }      // -1: no second residual
// Who can run beside whom: a tile enters block k + 1 behind level 5 of block k of all nine tiles of its neighbourhood,
// and a tile publishes level 5 behind E, its last read and last store of the block retired.  So while a tile is inside
// block k, each of its neighbours is inside block k too, or waits in front of block k or k + 1 holding nothing but
// weight slabs: a write of block k + 1 never meets a read of an earlier block, whichever buffer it goes to, and what is
// left are the hazards inside one block -- the single launch's.  Those are: x1..x4 (written into cur, read by the
// neighbours behind levels 1..4), and `out`, which a tile stores while its neighbours may still fetch halo pixels of
// every slice of cur: it must be another buffer.  The second residual is read from a tile's own pixels only, by the
// lanes that then store them, loads in front of stores.
constexpr bool chain_war_ok() {
    for (int r = 0; r < 3; ++r) {
        if (rdb_out_buf(r) == rdb_cur_buf(r)) return false;                                   // `out` against the neighbours' halo reads of cur
        if (rdb_res2_buf(r) >= 0 && rdb_res2_buf(r) != rdb_out_buf(r)) return false;          // in place: own pixels, load before store
        if (rdb_cur_buf((r + 1) % 3) != rdb_out_buf(r)) return false;                         // the next block runs where this one's result lies
    }
    return true;
}
static_assert(chain_war_ok(), "buffer rotation of chained blocks");
}  // namespace rdbs

}  // namespace nesr

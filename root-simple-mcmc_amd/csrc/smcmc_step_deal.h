// smcmc_step_deal.h -- the compile-time geometry of the step kernel (tiles of the moment fold, LDS layouts of the
// accepted point and of the decomposition, the Philox block of the accept word, the pieces of a step) and the plan that
// deals the fold's matrix instructions over the pieces.
//
// Plain C++17, no HIP: smcmc_kernels.hip.h includes it, and so do host programs (tests/cpp/step_deal_plan.C,
// tests/cpp/step_rowpairs_layout.C, tests/cpp/step_zero_row.C) that print the plan and the layout and let tests check
// their invariants.
#pragma once

namespace smcmc {

constexpr int kPiece = 16;   // columns of U consumed per scheduling region (8 x ds_read_b128)

template <int DP>
struct Geo {
    static constexpr int T = (DP + 1 + 15) / 16;   // 16-row tiles covering dims 0..DP-1 plus the ones row DP
    static constexpr int NT = T * (T + 1) / 2;     // lower-triangular tiles
    static constexpr int NB = (DP + 3) / 4;        // Philox blocks of 4 normals
    static constexpr int ROWS_MOMENTS = DP + 1;    // LDS rows of x: the dims and the ones row (zero rows are synthesized)
    // When at most 4 rows spill into the last 16-row tile (D = 50: rows 48, 49 and the ones row), that tile
    // row is folded with v_mfma_f64_4x4x4_4b_f64 instead (a quarter of the matrix-pipe time): its four
    // 4x4 blocks are (strip rows) x (columns 16 t + 4 blk ..), which lands exactly where register 0 of
    // tile (T-1, t) of the 16x16 scheme would, so the stored layout does not change.
    static constexpr bool STRIP = ((DP + 1) % 16 != 0) && ((DP + 1) % 16 <= 4);
    static constexpr int T16 = STRIP ? T - 1 : T;  // tile rows folded with 16x16x4
    static constexpr int NT16 = T16 * (T16 + 1) / 2;
};

// The register-array sizes the step kernels are built for, smallest first: SMCMC_FOR_EACH_DP of smcmc_kernels.hip.h, which
// holds a static_assert that the two lists agree.  Family DP serves the dimensions from the entry before it plus one up
// to DP (pick_dp of smcmc_host.hpp: the smallest family that holds the dimension).
constexpr int kDpFamilies[] = {7, 15, 31, 47, 50, 63};
constexpr int kNumDpFamilies = sizeof(kDpFamilies) / sizeof(kDpFamilies[0]);

// smcmc_accept_word of include/smcmc_detmath.h (a C header without constexpr), restated: the word of a step's stream
// that makes the Metropolis draw.  tests/cpp/step_rowpairs_layout.C holds the two against each other.
constexpr unsigned accept_word_of(unsigned dim) { return 2u * ((dim + 1u) / 2u); }

// Where the accept word of family DP lies.  FIXED: every dimension the family serves has it in the same Philox block of
// four words, BLOCK, and that block is one of the NB the proposal draws anyway -- a kernel may then take the word from
// that block alone, by `accept word & 3`, instead of testing every block against a run-time block number.
template <int DP>
struct AcceptBlock {
    static constexpr int lowest() {   // the smallest dimension the family serves
        int prev = 0;
        for (int f = 0; f < kNumDpFamilies; ++f) {
            if (kDpFamilies[f] == DP) return prev + 1;
            prev = kDpFamilies[f];
        }
        return 1;                     // not a family of the list: any dimension up to DP
    }
    static constexpr int LOWEST = lowest();
    static constexpr int BLOCK = (int)(accept_word_of((unsigned)DP) >> 2);
    static constexpr bool fixed() {
        for (int d = LOWEST; d <= DP; ++d)
            if ((int)(accept_word_of((unsigned)d) >> 2) != BLOCK) return false;
        return BLOCK < Geo<DP>::NB;
    }
    static constexpr bool FIXED = fixed();
};

// LDS image of the accepted point, x[row][lane] (lane = chain), 8-byte slots.
//   !PAIRS  row r, lane c at double r * kXStride + c: a stride of 2 (mod 32) doubles keeps both the lane = chain
//           ds_read / ds_write_b64 and the matrix-operand ds_read_b64 conflict-free.
//   PAIRS   rows 2p and 2p + 1 of a lane side by side: byte (r >> 1) * PAIR_STRIDE + 16 c + 8 (r & 1).  A lane reads or
//           writes its column in 16-byte accesses on one base address (offsets p * PAIR_STRIDE, within the 16-bit field),
//           each quarter-wave covering the 64 banks once.  The 32 bytes of padding per pair keep the fold's operand reads
//           conflict-free (ds_read_b64 of row 16 t + (lane & 15), lane 4 kk + (lane >> 4)): for a half-wave the dword
//           banks are 8 (r >> 1) + 4 c + 2 (r & 1) + {0, 1} (mod 64), all distinct.
// ROWS rows are held (the dims, and with the moment fold the ones row DP); PAIRS rounds that up to whole pairs.
constexpr int kXStride = 66;
template <int DP, bool MOMENTS, bool PAIRS>
struct XLayout {
    static constexpr int ROWS = MOMENTS ? Geo<DP>::ROWS_MOMENTS : DP;
    static constexpr int PAIR_STRIDE = 64 * 16 + 32;                   // bytes
    static constexpr int HELD = PAIRS ? (ROWS + 1) / 2 * 2 : ROWS;     // rows the image has room for
    static constexpr int LANE = PAIRS ? 2 : 1;                         // doubles from a lane to the next
    static constexpr int DOUBLES = PAIRS ? HELD / 2 * (PAIR_STRIDE / 8) : ROWS * kXStride;
    static constexpr int BYTES = DOUBLES * 8;
    // double index of row r in lane 0's column; lane c is LANE * c doubles further
    static constexpr int row(int r) { return PAIRS ? (r >> 1) * (PAIR_STRIDE / 8) + (r & 1) : r * kXStride; }
    static constexpr int offset(int r, int c) { return 8 * (row(r) + LANE * c); }   // bytes
    // The zero row: with the moment fold in row pairs the ones row DP has a partner, row DP + 1, that the prologue writes
    // +0 in every lane (idle ones too) and nothing writes again.  The fold's operand reads of tile rows past the ones
    // row go there: (+0) - (+0) = +0, the bits a select of 0.0 gave.  -1: the image holds no such row.
    static constexpr int ZERO_ROW = (PAIRS && MOMENTS && HELD > ROWS) ? ROWS : -1;
};

// LDS image of one table of the normal transform (64 or 128 entries of two doubles, gathered by ds_read_b128 at an index
// that differs from lane to lane and comes from a random word), COPIES times: copy c of entry k at byte
// k * STRIDE + 16 c, and lane l reads copy l & (COPIES - 1).  LDS has 64 banks of four bytes and serves a 16-byte read
// sixteen lanes at a time.  With 16 copies an entry's copies cover the 64 banks once and a lane's banks are
// 4 (l & 15) .. + 3 whatever its entry: any sixteen lanes with sixteen different l & 15 -- the contiguous quarters and
// the groups the hardware forms (tests/test_step_rowpairs_layout_cpu.py) -- read disjoint banks for ANY indices.  With 8
// copies two lanes of such a group share a copy, and only those two can meet in a bank: two-way at the most.  With one
// copy (the layout every other kernel keeps) any two lanes with different entries sixteen apart do.
// The lane's part of the address, lane_offset, does not change from step to step; the gather's address is one
// shift-and-add of the index, as it is for one copy.
template <int ENTRIES, int COPIES>
struct NormalTableLayout {
    static_assert(COPIES >= 1 && COPIES <= 16 && (COPIES & (COPIES - 1)) == 0, "a power of two, at most one per bank quad");
    static constexpr int ENTRY_BYTES = 16;
    static constexpr int STRIDE = ENTRY_BYTES * COPIES;     // bytes from an entry to the next
    static constexpr int SLOTS = ENTRIES * COPIES;
    static constexpr int BYTES = SLOTS * ENTRY_BYTES;
    static constexpr int shift() {                          // address = base + lane_offset + (index << SHIFT)
        int s = 0;
        while ((1 << s) < STRIDE) ++s;
        return s;
    }
    static constexpr int SHIFT = shift();
    static constexpr int copy_of(int lane) { return lane & (COPIES - 1); }
    static constexpr int lane_offset(int lane) { return ENTRY_BYTES * copy_of(lane); }
    static constexpr int offset(int copy, int k) { return k * STRIDE + ENTRY_BYTES * copy; }
    // staging: the prologue fills slot s (16 bytes at byte 16 s), s = 0 .. SLOTS - 1, with the source table's entry
    static constexpr int slot_offset(int s) { return ENTRY_BYTES * s; }
    static constexpr int slot_entry(int s) { return s / COPIES; }
};

// The copies each table gets in the headline kernels' workgroup (StepWorkgroupLds).  Sixteen of both do not fit beside
// four images of the accepted point.  Two lanes that share a copy meet in a bank unless they drew the same entry, one
// chance in 64 or in 128: either table with eight copies conflicts two-way in practically every pass, the counter cannot
// tell the two splits apart, and the listing and the clock decided (profiles/step_shared_tables_notes.md, which built
// the other splits with -D).
#ifndef SMCMC_NTAB_LOG_COPIES
#define SMCMC_NTAB_LOG_COPIES 8
#endif
#ifndef SMCMC_NTAB_ANGLE_COPIES
#define SMCMC_NTAB_ANGLE_COPIES 16
#endif
typedef NormalTableLayout<64, SMCMC_NTAB_LOG_COPIES> LogTableLayout;        // log table
typedef NormalTableLayout<128, SMCMC_NTAB_ANGLE_COPIES> AngleTableLayout;   // angle table over the half circle

// LDS image of the decomposition: row i keeps columns j0(i)..DP-1 (j0 = i rounded
// down to even for the triangular factor, 0 for a full matrix), padded to an even
// length so that every row starts 16-byte aligned (ds_read_b128 = two columns).
template <int DP, bool FULLU>
struct ULayout {
    static constexpr int DPE = DP + (DP & 1);       // DP rounded up to even
    static constexpr int j0(int i) { return FULLU ? 0 : (i & ~1); }
    static constexpr int len(int i) { return DPE - j0(i); }
    // closed form of sum_{r<i} len(r) (no loop: must fold once the caller's loops unroll)
    static constexpr int off(int i) {
        return FULLU ? i * DPE
                     : i * DPE - ((i & 1) ? 2 * (i / 2) * (i / 2) : 2 * (i / 2) * (i / 2 - 1));
    }
    static constexpr int SIZE = off(DP);
};

// LDS of the headline kernels' workgroup: kStepWaves wavefronts (chain groups kStepWaves b + w of block b), each with an
// image of the accepted point of its own (row pairs), behind them ONE decomposition and ONE set of tables.  More than
// 64 KB: dynamic shared memory, all offsets in bytes from its start.
constexpr int kStepWaves = 4;
constexpr int kLdsPerCU = 160 * 1024;
constexpr int step_group_of(int block, int wave) { return kStepWaves * block + wave; }
constexpr int step_blocks_for(int groups) { return (groups + kStepWaves - 1) / kStepWaves; }
template <int DP, bool MOMENTS>
struct StepWorkgroupLds {
    typedef XLayout<DP, MOMENTS, true> XL;
    static constexpr int round16(int n) { return (n + 15) / 16 * 16; }
    static constexpr int IMAGE_BYTES = round16(XL::BYTES);
    static constexpr int image(int wave) { return wave * IMAGE_BYTES; }
    static constexpr int US = kStepWaves * IMAGE_BYTES;
    static constexpr int US_BYTES = round16(8 * ULayout<DP, false>::SIZE);
    static constexpr int LOG = US + US_BYTES;
    static constexpr int ANGLE = LOG + LogTableLayout::BYTES;
    static constexpr int TOTAL = ANGLE + AngleTableLayout::BYTES;
    static constexpr bool FITS = TOTAL <= kLdsPerCU;   // one workgroup per CU: its LDS is the CU's
};

// The pieces (row, first column) that the rows of Philox block B contribute, in
// the order they are consumed.
template <int DP, bool FULLU, int B>
struct UPieces {
    typedef ULayout<DP, FULLU> UL;
    static constexpr int rows() { return (4 * B + 4 <= DP) ? 4 : (DP - 4 * B); }
    static constexpr int per_row(int i) { return (UL::len(i) + kPiece - 1) / kPiece; }
    static constexpr int count() {
        int n = 0;
        for (int q = 0; q < rows(); ++q) n += per_row(4 * B + q);
        return n;
    }
    static constexpr int COUNT = count();
    // pieces of the blocks before B (all rows < 4B)
    static constexpr int first_global() {
        int n = 0;
        for (int i = 0; i < 4 * B; ++i) n += per_row(i);
        return n;
    }
    static constexpr int row(int r) {
        int i = 4 * B;
        while (r >= per_row(i)) { r -= per_row(i); ++i; }
        return i;
    }
    static constexpr int col(int r) {
        int i = 4 * B;
        while (r >= per_row(i)) { r -= per_row(i); ++i; }
        return UL::j0(i) + r * kPiece;
    }
};

// LDS reads load_piece issues for the piece at column c
template <int DP, bool FULLU, int c>
constexpr int piece_reads() {
    int n = 0;
    for (int k = 0; k < kPiece / 2; ++k) n += (c + 2 * k < ULayout<DP, FULLU>::DPE) ? 1 : 0;
    return n;
}

// row ti of lower-triangular tile number `tile` (tile = ti (ti + 1) / 2 + tj, tj <= ti)
constexpr int tile_row(int tile) {
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
    return ti;
}

// ---- The deal of the fold's matrix instructions over the pieces of a step (triangular decomposition) ----
//
// A step has G pieces; behind the vector work of piece g is slot g, where matrix instructions of the moment fold issue.
// An FP64 matrix instruction holds the vector pipe (64 cycles for 16x16x4, 16 for the strip's 4x4x4) but not the issue of
// LDS reads, waits and scalar instructions: the non-vector instructions that follow a slot -- the operand prefetch of the
// next k-quad where the slot carries it, the next piece's reads and their wait -- issue in the shadow of the slot's
// LAST matrix instruction, four cycles each.  The model's score of a deal is
//     sum over instructions of min(4 x (non-vector instructions right behind it), duration - 4),
// and the plan maximises it under what the single-buffered operands (ma[], ms, raw[]) demand:
//   * k-quads in ascending order, all instructions of one before the operand preparation of the next (so every
//     accumulator tile sees ascending k: the sums keep their order and their bits);
//   * the first instruction of a k-quad is a 16x16, the prefetch of the next k-quad's operands goes to the end of that
//     slot, and the next k-quad starts in a later slot (a piece_ready lies between the prefetch and its use);
//   * at most one 16x16 per slot; strip instructions stand in front of it, or alone in a slot that gets no 16x16.
// Which slots get no 16x16 (there are G - 16 NT16 of them) is chosen by dynamic programming over the slots; the score of
// a 16x16 there is what the following piece's reads are worth, so the short pieces' boundaries go to the strip.
template <int DP>
struct StepDeal {
    typedef ULayout<DP, false> UL;
    static constexpr int NQ = 16;                          // k-quads: 64 chains, four per matrix instruction
    static constexpr int T = Geo<DP>::T;
    static constexpr int NT = Geo<DP>::NT;
    static constexpr int NT16 = Geo<DP>::STRIP ? Geo<DP>::NT16 : NT;
    static constexpr int NS = NT - NT16;                   // strip instructions per k-quad
    static constexpr int NM = NQ * NT;
    static constexpr int PREFETCH = T + (NS > 0 ? 1 : 0);  // LDS reads of one operand prefetch
    static constexpr int CYC16 = 64, CYCS = 16, ISSUE = 4; // cycles: 16x16x4, 4x4x4 4-block, one issue slot
    static constexpr int pieces() {
        int n = 0;
        for (int i = 0; i < DP; ++i) n += (UL::len(i) + kPiece - 1) / kPiece;
        return n;
    }
    static constexpr int G = pieces();
    static constexpr int SPARE = G - NQ * NT16;            // slots without a 16x16

    struct Plan {
        int first[G + 1];      // slot g issues instructions first[g] .. first[g + 1] - 1 of the sequence, in this order
        int kk[NM], tile[NM];  // the sequence: k-quad and accumulator tile (tile >= NT16: strip instruction tile - NT16)
        bool pf_after[NM];     // the operand prefetch of k-quad kk + 1 is issued right behind this instruction
        int fill[G];           // non-vector instructions behind slot g without a prefetch: LDS reads and one wait
        int score;
    };

    // Piece g + 1 opens with the reads of piece g + 2 and the wait for its own (the step loop of smcmc_kernels.hip.h); the
    // last piece of a Philox block opens with its wait alone, and behind it the next block starts with the reads of its
    // first piece and the wait for the normals' tables.
    static constexpr void fills(Plan& p) {
        int reads[G] = {};
        bool closes[G] = {};   // the last piece of its block
        int g = 0;
        for (int i = 0; i < DP; ++i) {
            for (int c = UL::j0(i); c < UL::DPE; c += kPiece, ++g) {
                for (int k = 0; k < kPiece / 2; ++k) reads[g] += (c + 2 * k < UL::DPE) ? 1 : 0;   // piece_reads<DP, false, c>()
                closes[g] = (c + kPiece >= UL::DPE) && (i % 4 == 3 || i + 1 == DP);
            }
        }
        for (g = 0; g < G; ++g) {
            if (g + 1 == G) p.fill[g] = 0;   // behind the last piece the step goes on with vector work
            else if (closes[g]) p.fill[g] = reads[g + 1] + 1;
            else if (closes[g + 1]) p.fill[g] = 1;
            else p.fill[g] = reads[g + 2] + 1;
        }
    }
    static constexpr int duration(int tile) { return tile < NT16 ? CYC16 : CYCS; }
    static constexpr int shadow(int nonvector, int tile) {
        const int a = ISSUE * nonvector, b = duration(tile) - ISSUE;
        return a < b ? a : b;
    }
    static constexpr void score(Plan& p) {
        p.score = 0;
        for (int g = 0; g < G; ++g) {
            for (int m = p.first[g]; m < p.first[g + 1]; ++m) {
                const int behind = (p.pf_after[m] ? PREFETCH : 0) + (m + 1 == p.first[g + 1] ? p.fill[g] : 0);
                p.score += shadow(behind, p.tile[m]);
            }
        }
    }

    // the deal the kernels without a plan keep: instruction m = kk NT + tile goes to piece m G / NM, prefetch behind tile 0
    static constexpr Plan make_uniform() {
        Plan p = {};
        fills(p);
        for (int g = 0; g <= G; ++g) p.first[g] = (int)(((long)g * NM) / G);
        for (int m = 0; m < NM; ++m) {
            p.kk[m] = m / NT;
            p.tile[m] = m % NT;
            p.pf_after[m] = (m % NT == 0) && (m / NT + 1 < NQ);
        }
        score(p);
        return p;
    }

    static constexpr Plan make() {
        static_assert(SPARE >= 0, "a 16x16 instruction per slot needs as many slots");
        static_assert(NS == 0 || NT16 >= 2, "strip instructions stand in front of a k-quad's later 16x16");
        Plan p = {};
        fills(p);
        // best[k][u]: the best score of the slots so far with k of them left without a 16x16 and u strip instructions of
        // the current k-quad standing alone in such slots.  what[g][k][u]: 0 = slot g gets a 16x16, 1 = a strip
        // instruction alone, 2 = nothing, as the step INTO that state.
        constexpr int K = SPARE + 1, U = NS + 1;
        int best[K][U] = {}, next[K][U] = {};
        signed char what[G][K][U] = {};
        for (int k = 0; k < K; ++k) for (int u = 0; u < U; ++u) best[k][u] = -1;
        best[0][0] = 0;
        for (int g = 0; g < G; ++g) {
            for (int k = 0; k < K; ++k) for (int u = 0; u < U; ++u) next[k][u] = -1;
            for (int k = 0; k < K; ++k) {
                for (int u = 0; u < U; ++u) {
                    if (best[k][u] < 0 || k > g) continue;
                    const int n16 = g - k;   // 16x16 instructions issued in the slots before g
                    if (n16 < NQ * NT16) {
                        const bool opens = n16 % NT16 == 0;
                        const bool carries = opens && n16 / NT16 + 1 < NQ;
                        const int v = best[k][u] + shadow(p.fill[g] + (carries ? PREFETCH : 0), 0);
                        const int u1 = opens ? 0 : u;
                        if (v > next[k][u1]) { next[k][u1] = v; what[g][k][u1] = (signed char)(0 + 4 * u); }
                    }
                    if (k + 1 < K) {
                        if (n16 > 0 && u < NS) {
                            const int v = best[k][u] + shadow(p.fill[g], NT16);
                            if (v > next[k + 1][u + 1]) { next[k + 1][u + 1] = v; what[g][k + 1][u + 1] = (signed char)(1 + 4 * u); }
                        }
                        if (best[k][u] > next[k + 1][u]) { next[k + 1][u] = best[k][u]; what[g][k + 1][u] = (signed char)(2 + 4 * u); }
                    }
                }
            }
            for (int k = 0; k < K; ++k) for (int u = 0; u < U; ++u) best[k][u] = next[k][u];
        }
        // walk back from the best end state (all 16x16 issued: k = SPARE)
        int choice[G] = {};
        {
            int k = SPARE, u = 0;
            for (int v = 0; v < U; ++v) if (best[k][v] > best[k][u]) u = v;
            for (int g = G - 1; g >= 0; --g) {
                const int w = what[g][k][u];
                choice[g] = w % 4;
                const int u0 = w / 4;
                if (choice[g] != 0) --k;
                u = u0;
            }
        }
        // the sequence: per k-quad its 16x16 in tile order, one per chosen slot; its strip instructions in order: those
        // that stand alone where the walk put them, the rest one each in front of the k-quad's second, third, ... 16x16
        // (the last 16x16 takes what remains)
        int alone[NQ] = {};
        for (int g = 0, n = 0; g < G; ++g) {
            if (choice[g] == 0) ++n;
            else if (choice[g] == 1) ++alone[(n - 1) / NT16];
        }
        int m = 0, n16 = 0, strips = 0, front = 0;   // strips, front: strip instructions of the current k-quad so far
        for (int g = 0; g < G; ++g) {
            p.first[g] = m;
            if (choice[g] == 2) continue;
            if (choice[g] == 1) {
                p.kk[m] = (n16 - 1) / NT16; p.tile[m] = NT16 + strips; ++m; ++strips;
                continue;
            }
            const int kq = n16 / NT16, t16 = n16 % NT16;
            if (t16 == 0) { strips = 0; front = 0; }
            else {
                int give = NS - alone[kq] - front;
                if (t16 + 1 < NT16 && give > 1) give = 1;
                for (int q = 0; q < give; ++q) { p.kk[m] = kq; p.tile[m] = NT16 + strips; ++m; ++strips; ++front; }
            }
            p.kk[m] = kq; p.tile[m] = t16; ++m;
            ++n16;
        }
        p.first[G] = m;
        // the prefetch of k-quad kk + 1: behind the last instruction of the slot that opens k-quad kk
        for (int g = 0; g < G; ++g) {
            for (int q = p.first[g]; q < p.first[g + 1]; ++q) {
                if (q % NT == 0 && p.kk[q] + 1 < NQ) p.pf_after[p.first[g + 1] - 1] = true;
            }
        }
        score(p);
        return p;
    }

    // what the kernel relies on (the host test checks the same on the printed plan)
    static constexpr bool valid(const Plan& p) {
        if (p.first[0] != 0 || p.first[G] != NM) return false;
        int pf_slot[NQ] = {};                    // slot of the prefetch of k-quad kk's operands (kk >= 1)
        for (int kk = 0; kk < NQ; ++kk) pf_slot[kk] = -1;
        for (int g = 0; g < G; ++g) {
            if (p.first[g + 1] < p.first[g]) return false;
            for (int m = p.first[g]; m < p.first[g + 1]; ++m) {
                // k-quads ascending, each complete before the next opens; every tile once per k-quad
                if (p.kk[m] != m / NT || p.tile[m] < 0 || p.tile[m] >= NT) return false;
                for (int q = (m / NT) * NT; q < m; ++q) if (p.tile[q] == p.tile[m]) return false;
                // the operands a k-quad opens with were fetched in an earlier slot: a piece_ready since
                if (m % NT == 0 && m > 0 && !(pf_slot[m / NT] >= 0 && pf_slot[m / NT] < g)) return false;
                if (p.pf_after[m]) {
                    // once per k-quad, behind its first instruction and in that instruction's slot
                    if (p.kk[m] + 1 >= NQ || pf_slot[p.kk[m] + 1] >= 0 || p.kk[m] * NT < p.first[g]) return false;
                    pf_slot[p.kk[m] + 1] = g;
                }
            }
        }
        for (int kk = 1; kk < NQ; ++kk) if (pf_slot[kk] < 0) return false;
        return true;
    }
};

// the plan of the headline kernels and the deal every other kernel keeps, scored by the same model
template <int DP>
inline constexpr typename StepDeal<DP>::Plan kStepDealPlan = StepDeal<DP>::make();
template <int DP>
inline constexpr typename StepDeal<DP>::Plan kStepDealUniform = StepDeal<DP>::make_uniform();

}  // namespace smcmc

/* Stand-alone driver of spgpu_amd/csrc/spmv_rules.h for tests/test_spmv_dispatch.py: what the ELL / HELL SpMV for rows as they come launches,
 * computed by the header the library's dispatch (ellpack_spmv.hip) uses, on operands that exist as addresses only.  Built with
 *   g++ -std=c++17 -O1 -Wall -Werror -fsanitize=undefined -fno-sanitize-recover=all
 * no argument: stdin, one Run call per line
 *   elemBytes hell form rows hackSize valStride idxStride maxNnz hint  offcM offrP offz offy  yGiven betaZero  said0 said1 said2 calls  frozen sweepKnob rowOrder
 *   off*: bytes by which the operand lies past a 16-byte boundary; said*: the three sample words, decoded; calls: as spgpuFormFeedback counts
 *   them; rowOrder: rIdx is given (and the deep split is off, so the call stays with the rows as they come).
 * stdout per line: "case <line number>", then
 *   call wideOk route wideIO noted   vote strips autoTile autoSweep probeBehind
 *   slab RPL PH HELL NT UNROLL PIPE TAIL STRIPS BLOCK TILE_BYTES TAIL_EVERY PACKED grid block   |   sweep VEC PACKS HELL HAS_BETA TAIL grid block
 *   probe RPL PH HELL STEP grid block   |   probe none
 * or "none" for a call that launches nothing (rows <= 0).
 * "constants": the header's constants by name.   "verdict": stdin lines "elemBytes rows said0 said1 said2" -> what spgpu?SpmvForm returns
 * for a matrix of rows > 0 whose probe left these words. */
#include "spmv_rules.h"

#include <cstdio>
#include <cstring>

using namespace spgpu;

static const void* at(int operand, long long off) { return (const void*)(((uintptr_t)(operand + 1) << 52) + (uintptr_t)off); }

static const char* routeName(SpmvRoute r)
{
    switch (r) {
    case SpmvRoute::Sweep: return "sweep";
    case SpmvRoute::Tiled: return "tiled";
    case SpmvRoute::Lean: return "lean";
    case SpmvRoute::Wide: return "wide";
    case SpmvRoute::NarrowTiled: return "narrow-tiled";
    default: return "narrow";
    }
}

static int constants()
{
#define SAY(name) printf(#name " %lld\n", (long long)(name))
    SAY(kRulesWave); SAY(kBlockThreads); SAY(kTailLanes); SAY(kTailUnroll); SAY(kTileBytes); SAY(kTileSpanNum); SAY(kTileSpanDen);
    SAY(kTiledBlockFp32); SAY(kTailEvery); SAY(kLeanMaxHint); SAY(kLeanMaxEll); SAY(kSweepLaneRows); SAY(kSweepPacks16);
    SAY(kSweepMaxBlocks); SAY(kAutoSweepRows); SAY(kProbeBlocks);
    SAY(kFormAuto); SAY(kFormGather); SAY(kFormStrips); SAY(kFormXtile); SAY(kFormSweep);
#undef SAY
    for (size_t eb : {4, 8, 16})
        printf("tileSpanLimit%zu %lld\nwideGroupRows%zu %d\n", eb, tileSpanLimit(eb), eb, wideGroupRows(eb));
    return 0;
}

static int verdicts()
{
    long long eb, rows, s0, s1, s2;
    while (scanf("%lld %lld %lld %lld %lld", &eb, &rows, &s0, &s1, &s2) == 5)
        printf("%d\n", formVerdict(countForms((int)s0, (int)s1, (int)s2), (size_t)eb, (int)rows));
    return 0;
}

int main(int argc, char** argv)
{
    if (argc > 1)
        return strcmp(argv[1], "constants") == 0 ? constants() : strcmp(argv[1], "verdict") == 0 ? verdicts() : 2;
    long long v[22];
    for (int line = 0;; ++line) {
        for (int k = 0; k < 22; ++k)
            if (scanf("%lld", v + k) != 1)
                return k == 0 ? 0 : 2;
        const size_t eb = (size_t)v[0];
        const bool hell = v[1] != 0, yGiven = v[13] != 0, betaZero = v[14] != 0, frozen = v[19] != 0, knob = v[20] != 0, rowOrder = v[21] != 0;
        const int rows = (int)v[3], hack = (int)v[4], maxNnz = (int)v[7], hint = (int)v[8], calls = (int)v[18];
        printf("case %d\n", line);
        if (rows <= 0) {
            printf("none\n");
            continue;
        }
        /* the steps of launchSlabFamily / voteForm / launchRowsAsTheyCome, without the handle */
        const bool wideOk = wideLayout(eb, hell, rows, hack, v[5], v[6], at(0, v[9]), at(1, v[10]));
        const int form = callerForm((int)v[2], wideOk, rowOrder);
        FormVote vote{};
        if (form == kFormAuto && votes(form, wideOk, eb))
            vote = autoVote(countForms((int)v[15], (int)v[16], (int)v[17]), calls, rows, eb, knob, rowOrder);
        else if (form != kFormSweep)
            vote = fixedVote(form, wideOk, eb);
        const SpmvChoice c = chooseRoute(form, wideOk, eb, hell, vote, hint, maxNnz, frozen);
        printf("call %d %s %d %d   vote %d %d %d %d\n", wideOk, routeName(c.route), narrowRoute(c.route) || wideIO(at(2, v[11]), yGiven ? at(3, v[12]) : nullptr), c.noted,
               vote.strips, vote.autoTile, vote.autoSweep, vote.probeBehind);
        if (c.route == SpmvRoute::Sweep) {
            const SweepShape s = sweepShape(eb);
            printf("sweep %d %d %d %d %d %u %d\n", s.vec, s.packs, hell, !betaZero, s.tail, sweepGrid(eb, rows), kBlockThreads);
        } else {
            const SlabShape s = slabShape(c.route, eb, c.strips, c.packed);
            printf("slab %d %d %d 1 %d %d %d %d %d %d %d %d %u %d\n", s.rpl, s.ph, hell, s.unroll, s.pipe, s.tail, s.strips, s.block, s.tileBytes,
                   s.tailEvery, s.packed, slabGrid(s, rows), s.block);
        }
        if (vote.probeBehind) {
            const ProbeShape p = probeShape(slabShape(wideOk && wideOf(eb) > 1 ? SpmvRoute::Wide : SpmvRoute::Narrow, eb));
            printf("probe %d %d %d %d %d %d\n", p.rpl, p.ph, hell, p.step, kProbeBlocks, kRulesWave);
        } else {
            printf("probe none\n");
        }
    }
}

// match_v2.hpp — exact rank-ordered placement (Fenzo scheduleOnce semantics, scheduler.clj:617-687) as a pipeline of
// window rounds.  Placement is sequential by definition — job i+1 sees job i's commitment — but one commitment changes
// ONE offer.  For a window of W consecutive jobs a round is three launches:
//
//   match_eval2    (grid = offer chunks x job groups; lane = job, offers walked in a wave-uniform loop over records staged in the
//                   wave's LDS): against the snapshot S of per-offer assignments at round start, every job gets the top-L
//                   feasible offers of each chunk (fitness desc, index asc), the first offers whose fitness exceeds
//                   good-enough, failure counts, and — for every (job, offer) — one bit "static constraints pass" (a ballot
//                   over the 64 jobs of the wave = one u64 per offer: colbits[offer][group]).  The two fp64 divides of the
//                   fitness are only executed for pairs whose cheap upper bound can still enter the lane's top-L.
//   match_merge2   (one wave per job): chunk lists -> the job's global top-LM / first-LG / failure counts.
//   match_resolve2 (ONE workgroup; wave 0 walks the window in rank order, SEGMENT by segment): the jobs the walk has to visit
//                   and their candidate lists are staged in LDS by walk position, a segment (up to MV_WSEG jobs) at a time;
//                   lanes own the offers committed to in this round ("touched", <= 64, state in registers) and an LDS table
//                   indexed by OFFER tells the owner lane of every offer.  For job j the winner under the current state S' is
//                       max( best UNTOUCHED offer under S , best TOUCHED offer re-evaluated under S' )
//                   and the first entry of j's list that is untouched — or touched and still feasible (its fitness only
//                   grew, so it dominates every untouched offer) — settles the left term.  A lane that opens an offer reads
//                   its record, snapshot state and colbits word from global memory (one round trip per opened offer; round 3
//                   staged every DISTINCT candidate of the window in an LDS slot table: 37 % of the workgroup's LDS, a hash
//                   build per round, and rounds that ended because the table was full).  When a segment is used up with the
//                   lists intact and lanes to spare the workgroup stages the next segment of the SAME evaluated window and the
//                   walker goes on with its lanes — no launch, no re-evaluation.  If a list runs out (truncated: more
//                   candidates may exist) or a 65th offer would be touched, the round ends there and the next re-snapshots.
//
// The result is bit-identical to the one-job-at-a-time sweep (match_serial) for every input; only speed depends on the shapes.
// Jobs of balanced / attribute-equals groups change the feasibility of UNTOUCHED offers when a cotask is placed, so a
// round never resolves a second member of such a group after the first one was placed.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "match_kernels.hpp"

// The parts, in their one valid order (each says in its first comment what it needs of those above it):
#include "match_v2_shapes.hpp"   // parameters and records: everything below is written in them
#include "match_v2_pack.hpp"     // once per call: the packed offers and jobs the rounds read
#include "match_v2_eval.hpp"     // a round's first launch; its constraint checks are the walk's too
#include "match_v2_merge.hpp"    // a round's second launch: reads the evaluation's chunk lists
#include "match_v2_resolve.hpp"  // a round's third launch: walks the merged lists, checks with the evaluation's functions
#include "match_v2_multi.hpp"    // the three launches for several pools: wraps the blocks of the three parts above
#include "match_v2_served.hpp"   // the walkers and their servers: built on PoolCtx and the same blocks

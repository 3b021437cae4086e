// match_v2_shapes.hpp — the window rounds' shapes and records: the COOK_MV_* build parameters and the constants derived from them, the packed
// offer and job records (OfferA / OfferB / OfferW, JobRec, JobCons), a pool's control block (WinCtl), the per-round log, the chunk lists of the
// evaluation (ChunkRecT) and the buffers of a call (V2Buf).  First part of match_v2.hpp: needs common.hpp and match_kernels.hpp (MatchIn,
// MatchState) only; every other part needs this one.
#pragma once

// waves per SIMD the eval kernels are compiled for (-DCOOK_EVAL_WAVES=n builds a tuning variant).  Four since round 5: the block's LDS
// is 27.6 KB (EvalLds), so a fourth wave per SIMD is there for the taking at 128 VGPRs; the compiler spills 39 (best fit) / 62 (good-enough
// launches) of the 158 / 161 registers it would like, and the cycle is still faster — eight pools 57.8 against 59.8 ms in lockstep pairs,
// 52.2 against 52.9 ms with served walkers (profiles/r05q_probe8.txt); 0 = the compiler's choice (three waves)
#ifndef COOK_EVAL_WAVES
#define COOK_EVAL_WAVES 4
#endif
#if COOK_EVAL_WAVES > 0
#define COOK_EVAL_OCCUPANCY COOK_WAVES_PER_SIMD(COOK_EVAL_WAVES)
#else
#define COOK_EVAL_OCCUPANCY
#endif

#ifndef COOK_MV_L
#define COOK_MV_L 8
#endif
constexpr int MV_L = COOK_MV_L;            // candidate list length per job and chunk (-DCOOK_MV_L=n builds a variant for tuning runs)
// Two LIST SHAPES of the merged lists (what the walk sees), chosen by the launch's template flag GE:
//   best fit (good-enough-fitness >= 1, the parity setting): 24 best-fit entries, no good-enough list.  A job's per-chunk top-L
//     lists determine its global top-LM exactly as long as no chunk has contributed all L of its entries (that chunk may hide an
//     (L+1)-th): the merge stops there and marks the list truncated.  Rounds per quarter-scale C4 pool against LM with nothing else
//     in the way (emulator): 12 -> 90 (the round-3 layout, 384 slots), 24 -> 62, 32 -> 60, 48 -> 59.
//   GE (good-enough-fitness < 1; config.clj:111 ships 0.8): there the "first offers above the threshold" list is the one that runs
//     out: every job of a window wants the SAME lowest-index offers above the threshold, so a round gets as far as that list reaches —
//     64 entries of it (one per lane of the walk), 32 best-fit entries for the jobs nothing clears the threshold for (rounds per quarter-scale
//     C4 pool at 0.8: 76 with round 3's lists of 16 / 12, 63 with 64 / 12, 41 with 64 / 24, 36 with 64 / 32).  The evaluation
//     hands the offers above the threshold over as a BIT per offer and chunk (complete: the merged list is exact to its last entry;
//     round 3's per-chunk lists of 12 cut the merged list at the first chunk with more than 12 such offers, usually the first).
// (64 since the end of round 5 — one entry per lane of the walk, 48 before: the reference's default K = 1000 4.79 -> 4.66 ms (7 -> 5 rounds per
//  pool: on an empty cluster best fit piles consecutive jobs onto the same offers and a list is stale after ~200 jobs), one C4 pool alone — one
//  GPU of the 8-GPU configuration — 40.9 -> 39.7 ms, eight pools on one GPU +- 0, C2 -1 %, C3 +1 %: profiles/r05zk_lm64_probe.txt,
//  r05y_variant_sweeps.txt; a staged job's LDS row grows from 613 to 805 bytes, segments get shorter and more)
#ifndef COOK_MV_LM
#define COOK_MV_LM 64
#endif
#ifndef COOK_MV_LM_GE
#define COOK_MV_LM_GE 32
#endif
template <bool GE>
struct VShape {
  static constexpr int LM = GE ? COOK_MV_LM_GE : COOK_MV_LM;  // merged best-fit entries per job
  static constexpr int LG = GE ? 64 : 0;           // merged good-enough entries per job
  static constexpr int LGS = GE ? 64 : 1;          // (array bound: never zero)
};
constexpr int MV_LM_MAX = COOK_MV_LM > COOK_MV_LM_GE ? COOK_MV_LM : COOK_MV_LM_GE, MV_LG_MAX = 64;
static_assert(VShape<false>::LM <= MV_LM_MAX && VShape<true>::LM <= MV_LM_MAX && VShape<true>::LG <= MV_LG_MAX, "buffer sizing");
static_assert(MV_LM_MAX <= 64 && MV_LG_MAX <= 64, "the walk holds one merged-list entry per lane");
#ifndef COOK_MV_OCW
#define COOK_MV_OCW 32
#endif
constexpr int MV_OCW = COOK_MV_OCW;        // offers per eval wave (a power of two <= 64; -DCOOK_MV_OCW=n builds a tuning variant)
#ifndef COOK_MV_EW
#define COOK_MV_EW 4
#endif
constexpr int MV_EW = COOK_MV_EW;          // waves per eval block (same 64 jobs, consecutive offer sub-chunks)
constexpr int MV_OCB = MV_OCW * MV_EW;     // offers per eval block
constexpr int MV_T = COOK_WAVE;            // touched offers per round = lanes of the walking wave
#ifndef COOK_MV_RTHREADS
#define COOK_MV_RTHREADS COOK_SHAPE(768, 256)  // (the emulated tests: fewer fibers per block; the strides are blockDim.x either way)
#endif
constexpr int MV_RTHREADS = COOK_MV_RTHREADS;  // threads of the resolve workgroup: the staging is parallel over them, wave 0 walks
// Jobs staged in LDS per SEGMENT of the walk (at most; the offer-owner table shares the LDS: resolve_wseg).  The emulated tests: small,
// so that small inputs run many segments and rounds.
#ifndef COOK_MV_WSEG
#define COOK_MV_WSEG COOK_SHAPE(384, 96)
#endif
constexpr int MV_WSEG = COOK_MV_WSEG;
// Largest window the TILE path of the evaluation serves (rows of the eval grid = MV_WEVAL / 64): a round evaluates up to that many
// jobs against one snapshot and the walk consumes them segment by segment.
#ifndef COOK_MV_WEVAL
#define COOK_MV_WEVAL COOK_SHAPE(960, 256)
#endif
constexpr int MV_WEVAL = COOK_MV_WEVAL;
constexpr int MV_JG = MV_WEVAL / 64;       // job groups (waves of jobs) of such a window = rows of the eval grid
static_assert(MV_WEVAL % 64 == 0 && MV_JG >= 1, "whole job groups");
// A window may grow to MV_WLONG jobs once next to nothing of it has to be WALKED: when the cluster is full almost every job is
// settled in the parallel phase of the resolve kernel (no feasible offer under the snapshot, however the jobs before it fare) and
// needs no LDS at all.  One C4 pool spent 152 of its 604 rounds resolving 512 such jobs each; with long windows that tail takes
// about 20 rounds.
// (round 5: 10 240 instead of 2 560 — the tail of a C4 pool, 60 000 jobs that no offer can take any more, is 5 rounds instead of 25; one pool
//  42.1 -> 41.1 ms, eight pools 52.2 -> 50.7 ms; 5 120 / 20 480 measured 41.4 / 41.4 and 51.1 / 50.7: profiles/r05w_wlong_sweep.txt)
#ifndef COOK_MV_WLONG
#define COOK_MV_WLONG COOK_SHAPE(10240, 1024)
#endif
constexpr int MV_WLONG = COOK_MV_WLONG;
constexpr int MV_JGL = MV_WLONG / 64;      // job groups of a long window (stride of colbits)
static_assert(MV_WLONG % 64 == 0 && MV_WLONG >= MV_WEVAL && MV_WLONG < 65536, "JobL::b is 16 bits");
static_assert(MV_OCW <= COOK_WAVE, "one lane stages one offer");
static_assert(MV_OCW == 64 || MV_OCW == 32 || MV_OCW == 16 || MV_OCW == 8, "a wave's alive bits are an aligned slice of one 64-bit word");

struct OfferA {  // resources of an offer (offer.clj:55-61) + Fenzo's running view; 48 B, read wave-uniformly
  double oc, om;          // lease cpus / mem
  double rc, rm;          // resources of tasks Fenzo tracks as running on the host
  double inv_dc, inv_dm;  // 1 / (oc + rc), 1 / (om + rm): only for the pruning bound, never for the fitness itself
};
struct OfferB {  // what the cheap constraint checks need; 32 B
  uint32_t host, gpu_model;
  double gpu_count;
  int32_t run_count, task_slack;  // task_slack = COOK_MAX_TASKS_PER_HOST - COOK_NUM_TASKS_ON_HOST (INT_MAX when absent)
  uint32_t flags, pad;            // bit0 kubernetes VM, bit1 host is in the rebalancer's reserved set, bit2 the host's "gpus" map has
                                  // several entries (gpu_model = one of them; the constraint reads the table)
};
// What a lane of the placement walk needs when it becomes the owner of an offer, as ONE cache line: the offer's record and its state as
// of the last round's end (the resolve kernel keeps the state fields current next to MatchState's arrays, which the evaluation reads).
// Opening an offer was five cache lines (OfferA, OfferB, three state arrays) and ~1 000 cycles of the one walking wave per opened offer.
struct alignas(128) OfferW {
  double oc, om, rc, rm, inv_dc, inv_dm;  // = OfferA
  uint32_t host, k8s;                     // OfferB::host, flags bit 0
  int32_t run_count, task_slack;
  double ac, am;                          // assigned by the rounds so far
  int32_t acount;
  uint32_t pad[11];
};
static_assert(sizeof(OfferW) == 128, "one cache line per offer");
struct JobRec {  // one considerable job in match order; 40 B
  double c, m, g;
  uint32_t gpu_model;
  int32_t reserved_host;
  uint32_t group;  // COOK_NONE_U32 or group id
  uint32_t flags;  // bit0 has constraints that need the slow static check, bit1 member of a constrained group,
                   // bits 8..9 group type
};
constexpr uint32_t JF_SLOW = 1u, JF_GROUPED = 2u, JF_FASTC = 4u, JF_XRES = 8u;  // JF_XRES: asks for ports / named scalars
// The common job constraints in a form the eval loop checks from registers + LDS only: up to MV_NC user-defined EQUALS
// pairs on attribute keys < MV_NA (or HOSTNAME) and up to MV_NC novel-host entries.  Jobs with more, or with a disk /
// estimated-completion / checkpoint constraint, carry JF_SLOW and go through static_pass (global-memory CSR walk).
constexpr int MV_NC = 4;   // fast constraint slots per kind
constexpr int MV_NA = 8;   // attribute keys staged in LDS per offer
constexpr int MV_FH = 8;   // hosts a unique-group job must avoid, kept in registers per tile
struct JobCons {
  uint32_t eq_key[MV_NC], eq_val[MV_NC], novel[MV_NC];
  uint32_t n_eq, n_novel;
};

struct WinCtl {
  unsigned head;          // first unresolved job
  unsigned wcur;          // window size for the next round
  unsigned rounds;
  unsigned matched;
  unsigned head_matched;  // job 0 was matched
  unsigned stop_list, stop_full, stop_group, stop_window;  // why rounds ended (statistics): a truncated list ran out, 64 offers touched,
                                                           // second member of a group whose constraint can open offers, window used up
  unsigned segments;      // segments staged (the excess over the rounds that walked anything = continuations without a launch)
  unsigned touched_sum;   // sum over rounds of touched offers
  unsigned visited_sum;   // sum over rounds of jobs the walk had to visit (the rest were settled in parallel)
  unsigned long long t_setup, t_seq;  // resolve kernel: ticks (100 MHz wall clock) spent staging / in the sequential phase
  unsigned trunc_lists;   // walked jobs whose merged list carried the truncated flag (the merge stopped on a full chunk list)
  unsigned wgrow_pct;     // next window = this percentage of what the round resolved (window ended early) / of the window (it did not)
  unsigned wlong_cap;     // largest window the launch sequence allows (MV_WLONG, or MV_WEVAL when long windows are switched off)
  unsigned no_retire;     // the next round gives no lanes of dead offers away (the last one used few lanes: see resolve_round)
#ifdef COOK_WALK_PROF  // measurement build: shader cycles / jobs of the walk by outcome (0 shortcut, 1 touched offer wins, 2 new lane,
                       // 3 walked and unmatched, 4 member of a constrained group, 5 exact path ran)
  unsigned long long prof_cyc[8];
  unsigned prof_cnt[8];
#endif
};

struct RoundLog {  // one record per round (diagnostics; only written when V2Buf::round_log is set)
  unsigned head, wcur, resolved, n_list, touched, stop, matched, setup_ticks, seq_ticks, segments;
  // what the round was GIVEN, as checksums (only computed when a log is kept): the merged lists' summary words of the window, the offer
  // state and the alive bits the window was evaluated against, the static-constraint bits of the window's job groups
  unsigned h_cinfo, h_state, h_alive, h_col;
};
constexpr unsigned MV_ROUND_LOG_CAP = 8192;

// One offer chunk's candidates for one job, as ONE aligned record (128 bytes for best fit, 144 with the good-enough bits) that the
// evaluating lane writes and the merging lane reads in 16-byte pieces.
template <bool GE>
struct alignas(16) ChunkRecT {
  double fit[MV_L];         // fitness desc, offer index asc
  int idx[MV_L];            // -1 = no entry
  unsigned long long gm[GE ? MV_EW : 2];  // (GE) bit i of word w: the fitness of offer chunk * MV_OCB + w * MV_OCW + i exceeds good-enough
  unsigned cnt[4];          // n | nge << 8, offers failing on resources / constraints / zero fitness
};
static_assert(sizeof(ChunkRecT<false>) % 16 == 0 && sizeof(ChunkRecT<true>) % 16 == 0, "ChunkRec is moved in 16-byte pieces");
static_assert(offsetof(ChunkRecT<false>, cnt) + 16 == sizeof(ChunkRecT<false>) && offsetof(ChunkRecT<true>, cnt) + 16 == sizeof(ChunkRecT<true>),
              "the counts are the record's last 16-byte piece");
// an empty list is stored from this piece on (chunk_store): the merge reads n = 0 and ignores the rest
template <bool GE>
constexpr unsigned chunk_count_piece() { return (unsigned)(offsetof(ChunkRecT<GE>, cnt) / 16); }
// (chunk_store: platform.hpp)

struct V2Buf {
  RoundLog* round_log;
  unsigned split_max;  // cap of eval_split (1 = never cut a wave's offer batch)
#ifdef COOK_EVAL_TRACE
  unsigned long long* eval_trace;  // timing study build: per eval block [start, end] ticks of the 100 MHz clock + HW_ID
#endif
  const OfferA* oa;
  const OfferB* ob;
  OfferW* ow;          // [M] the walk's one-line records (state fields written by the resolve kernel)
  const JobRec* jr;
  const JobCons* jcons;  // [K] fast constraint slots of the jobs flagged JF_FASTC
  void* prec;          // [wlong][C]     chunk lists: one ChunkRecT<GE> per (job of the window, offer chunk)
  uint64_t* colbits;   // [M][JGL]       static-constraints-pass bit of (offer, job of the window)
  unsigned* jfh;       // [wlong][MV_FH + 2]  group members: the hosts their cotasks occupy under the snapshot (unique groups), how many
                       //                (int: -1 not gathered, -2 more than MV_FH), the group's last placed job — what the walk's fast
                       //                path needs, gathered ONCE by the evaluation (the tile of chunk 0 writes it)
  double* cand_fit;    // [wlong][LM]
  int* cand_idx;       // [wlong][LM]
  int* ge_idx;         // [wlong][LG]
  uint32_t* cinfo;     // [wlong][4]     ncand | nge << 8 | truncated << 16 | good-enough list truncated << 17, c1, c2, c4
  WinCtl* ctl;
  const MatchIn* in_dev;  // the MatchIn of this call in device memory (the walk only needs it for constrained groups)
  unsigned C;          // eval blocks along the offers
};

// launch_plan.h -- the launch schedule of the detector: the size classes of the quad fit (plan_classes, at creation), their work
// lists (plan_work_layouts, whenever the point or cluster capacity changes) and what one submission launches, with which grids,
// in which order and on which streams (plan_launch, every launch: it reads the pair-table capacity, which grows).  detector.hip
// executes the plans.  Plain C++ without HIP, so that tests/test_launch_plan_cpu.py compiles it on the host; hence FqWorkLayout,
// the kernels' argument, lives here too.  No result depends on the launch set, the instances, grids, order or streams: only
// the speed does.
#pragma once
#include <stdint.h>

#include "../../include/apriltag_amd.h"         // AMDAT_SUCCESS, AMDAT_BATCH_TOO_LARGE
#include "../../include/apriltag_amd_debug.h"   // AMDAT_PATH_*

// Size classes of the quad fit.  Class 0 runs k_fit_small<2>; class 1 is an empty slot (its K = 4 instance measured no gain,
// DESIGN.md section 5); classes FQ_C0 .. run k_fit_quads with 64 ... 1024 threads.
#define FQ_NCLS 7
#define FQ_C0 2
#define FQ_NT_BIG 1024   // threads of the largest class: one workgroup fills a CU (16 waves, 4 per SIMD)

// Work lists of the quad fit (k_cluster_select buckets the kept clusters, class c takes lo[c] < count <= hi[c]).
struct FqWorkLayout {
  int lo[FQ_NCLS], hi[FQ_NCLS];
  uint32_t off[FQ_NCLS], cap[FQ_NCLS];   // item range of class c inside the work array
};

// Side streams of the quad fit.  Three, as in every earlier round: a captured submission with six parallel branches (five side
// streams + the submission stream) crashed inside hipGraphLaunch (hip::Graph::UpdateStreams, ROCm 7.2) in about one of seven
// 300-case fuzz runs; with four branches it never has.
#define FQ_NAUX 3

enum FqKernel { FQ_EMPTY = 0, FQ_SMALL, FQ_QUADS };   // no kernel; k_fit_small<2>; k_fit_quads<nt>

// One size class: workgroup size, LDS key capacity, cluster sizes (lo, hi], persistent grid, scratch slot size (points), clusters
// taken from the work list per atomic, kernel.
struct FqClassSpec {
  int nt, sort_cap, lo, hi;
  unsigned grid;
  int slot_cap, pop;
  FqKernel kernel;
};
struct FqClassTable {
  FqClassSpec cls[FQ_NCLS];
  int prefilter_class;      // first class whose clusters go through k_fit_prefilter (those above 2048 points)
  int max_cluster_points;   // DetParams::max_cluster_points
};

// Persistent workgroups per CU of the one-wave classes (they fill four waves per SIMD when alone on a CU) and of the 128-thread class.
constexpr unsigned FS_GRID_K2 = 16, FQ_GRID_64 = 16, FQ_GRID_128 = 8;

// One wave per small cluster, bigger workgroups and LDS key arrays above; persistent grids sized to the chip (CUs x workgroups
// that fit one CU) but not beyond what a submission of max_batch frames can feed.
// The two large classes need most of a CU's LDS for their key arrays, so they cannot share a CU with the other classes'
// persistent workgroups: they run first and alone, at the 128-register budget of the other classes -- clusters above 8192 points
// in 1024-thread workgroups (16 waves, one workgroup per CU), then 4096..8192 points in 512-thread workgroups, two per CU.  (With
// 512 threads at twice the registers and no room for a neighbour the largest clusters used to run at a quarter of the chip's
// occupancy, mostly at the end of the stage: 17 ms of wall time for 4 % of the stage's instructions.)
inline FqClassTable plan_classes(int max_cluster_points, bool split_moments, unsigned cus, uint32_t max_batch) {
  auto grid = [&](unsigned per_cu, unsigned per_frame) { return per_cu * cus < per_frame * max_batch ? per_cu * cus : per_frame * max_batch; };
  // Class boundaries: the one-wave class has no workgroup barriers at all and runs closest to the VALU issue rate (82 % against
  // 53-57 % for the 128- and 256-thread classes), so it takes clusters up to 768 points, the most its 16 workgroups per CU can hold
  // in LDS (9 KB each); measured 16.1 ms (256 / 1024) -> 15.5 (512 / 1024) -> 15.35 (768 / 2048); 896 and 1024 are slower again
  // (fewer resident workgroups).
  // Clusters per pop: one atomic per cluster saturates the list cursor (one-wave class: 18.7 ms), chunks of 16 / 8 / 2 leave
  // workgroups with up to 16 clusters of work while others have drained the list (15.4 ms); 4 / 2 / 1: 15.0.
  // The smallest class runs k_fit_small (kernels_quad_small.h): clusters up to 128 points, whose keys and sweep state fit a
  // wave's registers and whose cumulative moments fit LDS.  It exists on the two-double path only (working images up to
  // 2048 x 2048); otherwise its range is empty and the one-wave class starts at 0.
  // (a "latency layout" for small-batch handles -- about three times the threads per cluster: 64 up to 256 points, 128 up to 768,
  // 256 up to 2048, 512 up to 8192 -- measured slower on one-frame submissions, 0.36 against 0.28 ms for the stage: the larger
  // workgroups' barriers cost more than the shorter per-lane runs save)
  const int sb = split_moments ? 128 : 0;
  FqClassTable t;
  t.cls[0] = {64, 0, 0, sb, grid(FS_GRID_K2, 4096), sb, 4, FQ_SMALL};
  t.cls[1] = {64, 0, sb, sb, 0, 0, 0, FQ_EMPTY};
  t.cls[2] = {64, 768, sb, 768, grid(FQ_GRID_64, 4096), 768, 4, FQ_QUADS};
  t.cls[3] = {128, 2048, 768, 2048, grid(FQ_GRID_128, 1024), 2048, 2, FQ_QUADS};
  t.cls[4] = {256, 4096, 2048, 4096, grid(4, 256), 4096, 1, FQ_QUADS};
  t.cls[5] = {512, 8192, 4096, 8192, grid(2, 64), 8192, 1, FQ_QUADS};
  t.cls[6] = {FQ_NT_BIG, 16384, 8192, 0x7FFFFFFF, grid(1, 16), max_cluster_points > 8193 ? max_cluster_points : 8193, 1, FQ_QUADS};
  static_assert(FQ_C0 + 5 == FQ_NCLS, "class table");
  if (max_cluster_points > 16384 && max_cluster_points <= 18432) t.cls[6].sort_cap = (max_cluster_points + 63) & ~63;
  t.prefilter_class = FQ_C0 + 2;
  t.max_cluster_points = max_cluster_points;
  return t;
}

// The cluster sizes (lo, hi] class c takes on a launch set.  A latency submission buckets every cluster up to the one-wave
// class's bound into that class and launches no k_fit_small (plan_launch).  Kept clusters have at least 24 points
// (DetParams::min_cluster_points).
inline void class_range(const FqClassTable& t, int c, bool latency, int* lo, int* hi) {
  *lo = t.cls[c].lo < 23 || (latency && c <= FQ_C0) ? 23 : t.cls[c].lo;
  *hi = latency && c < FQ_C0 ? 0 : t.cls[c].hi;
}
// Class c can be handed a cluster on a launch set: it launches if and only if this holds, and has scratch if it holds on either set.
inline bool class_sees_clusters(const FqClassTable& t, int c, bool latency) {
  int lo, hi;
  class_range(t, c, latency, &lo, &hi);
  return t.cls[c].kernel != FQ_EMPTY && lo < hi && lo < t.max_cluster_points;
}

// The work layouts of both launch sets over one work array: every class's list holds what a frame of pcap points and ccap clusters
// can put there on either set (the latency set's lower bounds are the smaller ones).  AMDAT_BATCH_TOO_LARGE where an offset or a
// cursor would not fit 32 bits.
struct FqWorkLayouts {
  FqWorkLayout all, latency;
  uint64_t words;   // items in the work array
};
inline int plan_work_layouts(const FqClassTable& t, uint32_t pcap, uint32_t ccap, uint32_t max_batch, FqWorkLayouts* out) {
  uint64_t off = 0;
  for (int k = 0; k < FQ_NCLS; k++) {
    const FqClassSpec& c = t.cls[k];
    class_range(t, k, false, &out->all.lo[k], &out->all.hi[k]);
    class_range(t, k, true, &out->latency.lo[k], &out->latency.hi[k]);
    const uint32_t per_frame = pcap / (uint32_t)(out->latency.lo[k] + 1) + 1;
    const uint64_t cap = c.hi <= c.lo ? 16 : (uint64_t)max_batch * (per_frame < ccap ? per_frame : ccap);   // (an empty class keeps a token range)
    if (cap > 0x7FFFFFFFull || off + cap > 0xFFFFFFFFull) return AMDAT_BATCH_TOO_LARGE;   // offsets and cursors are 32-bit
    out->all.off[k] = out->latency.off[k] = (uint32_t)off;
    out->all.cap[k] = out->latency.cap[k] = (uint32_t)cap;
    off += cap;
  }
  out->words = off;
  return AMDAT_SUCCESS;
}

// Working pixels per submission below which a submission is about latency, not throughput (AMDAT_PATH_AUTO): the node's one-frame
// calls, up to eight 1080p frames.  Every cluster is a workgroup's only one, the stage ends with its longest chain, and a launch more
// costs more than k_fit_small's shorter chain per small cluster saves (measured: 0.54 against 0.47 ms per one-frame call).
constexpr uint64_t LATENCY_MAX_PX = 16ull << 20;
// k_cc_local<16> below this many (eight 1080p frames: 0.089 ms with four waves per tile against 0.123 with sixteen -- the chip is
// full by then; four frames: 0.068 either way)
constexpr uint64_t CC_WIDE_MAX_PX = 8ull << 20;
// without the prefilter, the two large classes run first from this many on (about 32 1080p working images; below that the two
// extra dependent launches cost more than the placement gains -- 64 half-resolution frames measured 3.00 vs 2.88 ms)
constexpr uint64_t LARGE_FIRST_MIN_PX = 64ull << 20;

// The launch set of a submission of n frames: by its size, or pinned by amdAprilTagsDebugSetSubmissionPath, so that the parity
// tests can put BOTH sets under the oracle at any frame count.
inline bool latency_set(uint32_t n, int W, int H, int path_mode, uint64_t limit = LATENCY_MAX_PX) {
  if (path_mode != AMDAT_PATH_AUTO) return path_mode == AMDAT_PATH_LATENCY;
  return (uint64_t)n * (uint64_t)W * (uint64_t)H < limit;
}

enum FitStepKind { FIT_PREFILTER, FIT_CLASS, FIT_FORK };
constexpr int FIT_MAIN = -1;   // FitStep::stream: the submission stream
struct FitStep {
  FitStepKind kind;
  int cls;          // FIT_CLASS: the class
  unsigned grid;    // FIT_PREFILTER, FIT_CLASS: workgroups
  int pop;          // FIT_CLASS: clusters per pop
  bool compact;     // FIT_CLASS: pops from the prefilter's compact list
  int stream;       // FIT_MAIN or side stream 0 .. FQ_NAUX - 1; FIT_FORK: the side streams wait for the submission stream here
};
struct LaunchPlan {
  bool latency;                 // the launch set: AMDAT_PATH_LATENCY or AMDAT_PATH_THROUGHPUT
  int cc_waves;                 // k_cc_local<cc_waves>
  bool border_per_wave;         // k_cc_border<border_per_wave>
  unsigned cc_root_grid;        // k_cc_sizes, k_cc_resolve: (cc_root_grid, 1, n)
  int select_chunks;            // k_cluster_select: chunks per block, grid (select_grid, 1, n), latency ? latency : all layout
  unsigned select_grid;
  bool prefilter;               // k_fit_prefilter<prefilter_nt> runs (one FIT_PREFILTER step) for the classes from prefilter_first
  int prefilter_nt, prefilter_first;
  int nsteps;
  FitStep steps[FQ_NCLS + 2];   // the quad fit in enqueue order; the side streams join the submission stream after the last
  unsigned decode_grid;         // k_decode_wave: (decode_grid, n)
};

// The launches of one submission of n frames of W x H working pixels on a handle with a pair table of hcap slots.
inline LaunchPlan plan_launch(const FqClassTable& t, uint32_t n, int W, int H, uint32_t hcap, int path_mode, unsigned cus, bool prefilter_built) {
  LaunchPlan p = {};
  p.latency = latency_set(n, W, H, path_mode);
  // the frame count the heuristics see (chunks of k_cluster_select, clusters per pop): a pinned path takes the values of the
  // submissions that path is for, whatever the real count
  const uint32_t hframes = path_mode == AMDAT_PATH_THROUGHPUT ? (n < 64u ? 64u : n) : path_mode == AMDAT_PATH_LATENCY ? (n > 8u ? 8u : n) : n;
  // sixteen waves per tile: a quarter of the rows per lane (latency, not throughput)
  p.cc_waves = latency_set(n, W, H, path_mode, CC_WIDE_MAX_PX) ? 16 : 4;
  // one list append per block on the latency set, per wave (no barriers) on the throughput set
  p.border_per_wave = !p.latency;
  const unsigned gr = (unsigned)(((uint64_t)W * (uint64_t)H / 16 + 255) / 256);
  p.cc_root_grid = gr < 1 ? 1 : (gr > 1024 ? 1024 : gr);
  p.select_chunks = hframes >= 16 ? 4 : 1;   // (SEL_CHUNKS, kernels_cluster.h)
  p.select_grid = (hcap + 1024u * (unsigned)p.select_chunks - 1) / (1024u * (unsigned)p.select_chunks);

  // Cheap exits of the large classes (bounding box, border direction, sector test) at full occupancy, ahead of their persistent
  // workgroups, which pop the survivors from the compact lists it writes.  A latency submission (the node's one-frame calls) is
  // over when its slowest chain is: there the 256-thread class starts at once beside the small classes (its in-kernel test after
  // the first walk still drops most of its clusters) and only the two largest classes wait for the prefilter -- prefilter, then
  // the survivors' sort, was the longest chain.  One cluster per CU-wide workgroup there (latency), one per wave otherwise.
  p.prefilter = prefilter_built && t.max_cluster_points > t.cls[t.prefilter_class].lo;
  p.prefilter_first = p.latency ? t.prefilter_class + 1 : t.prefilter_class;
  p.prefilter_nt = p.latency ? 1024 : 64;
  const unsigned pf_cap = 256u * n, pf_grid = (p.latency ? 2u : 32u) * cus;
  const unsigned pf_grid_n = pf_grid < pf_cap ? pf_grid : pf_cap;

  auto step = [&](FitStepKind kind, int stream) -> FitStep& {
    FitStep& s = p.steps[p.nsteps++];
    s = {kind, -1, 0, 0, false, stream};
    return s;
  };
  auto fork = [&]() { step(FIT_FORK, FIT_MAIN); };
  auto prefilter = [&]() { step(FIT_PREFILTER, FIT_MAIN).grid = pf_grid_n; };
  // classes that see no cluster launch nothing and take no stream
  auto launch = [&](int c, int stream) -> bool {
    if (!class_sees_clusters(t, c, p.latency)) return false;
    const FqClassSpec& cl = t.cls[c];
    FitStep& s = step(FIT_CLASS, stream);
    s.cls = c;
    // (latency set: the one-wave class's sixteen workgroups per CU -- the throughput grid -- leave the 128- and 256-thread classes'
    // workgroups waiting for slots; eight per CU: one 1080p frame 0.395 -> 0.383 ms, four 0.682 -> 0.650, eight 1.028 -> 1.00;
    // six: the same; four: 0.397 / 0.723 / 1.12.  The 128-thread class gets two per CU there, the 256-thread class one.)
    const unsigned lat_per_cu = c == FQ_C0 ? 8u : c == FQ_C0 + 1 ? 2u : c == FQ_C0 + 2 ? 1u : 0u;
    s.grid = p.latency && lat_per_cu && cl.grid > lat_per_cu * cus ? lat_per_cu * cus : cl.grid;   // (n < max_batch: the handle's grid)
    // a small submission spreads its clusters over the workgroups one by one (latency); large ones pop in chunks
    const int nh16 = (int)(hframes / 16u);
    s.pop = cl.pop < nh16 ? cl.pop : (nh16 < 1 ? 1 : nh16);
    s.compact = p.prefilter && c >= p.prefilter_first;
    return true;
  };

  // The classes are independent (they only append to the quad list).  Every class's persistent grid can fill the chip's register
  // file by itself, so whichever workgroups are placed first stay until their list is empty, and the stage is work-conserving
  // whatever the order of the three small classes (17.97 - 18.34 ms over five stream assignments).  The two large classes are
  // different: their workgroups only find room on (half-)empty CUs.  Next to the small classes they were placed last and ran at
  // the end of the stage at a quarter of the chip's occupancy, so a throughput-sized submission runs them first, one after the
  // other on the submission stream, and the small classes start when both are done: 16.9 -> 15.8 ms.  (Queuing the largest class
  // on a stream of its own next to the second one cost 0.9 ms: its queue sat stalled until the scheduler looked at it again.)
  // A latency submission leaves most of the chip empty either way: all classes start together.
  if (p.prefilter) {
    // The prefilter runs first and alone (a fraction of a millisecond at full occupancy; started beside the small classes it
    // starved behind their persistent workgroups and finished last).  The two largest classes need (half) a CU's LDS per
    // workgroup: queued beside the small classes' persistent grids they found no room until those drained -- the 1024-thread
    // class, 15 us of work, sat behind k_fit_small for 1.4 ms whenever it lost that race (profiles/r05_v4_fit_timeline.txt) -- so a
    // throughput-sized submission runs them right behind the prefilter, on the empty chip, and everything else starts when they
    // are through (their lists hold the prefilter's few survivors).  On the latency set the fork comes first: the classes below
    // the prefilter start at once on the side streams, beside it.
    if (!p.latency) {
      prefilter();
      for (int c = p.prefilter_first + 1; c < FQ_NCLS; c++) launch(c, FIT_MAIN);
    }
    fork();
    if (p.latency) prefilter();
    for (int c = p.prefilter_first; c < (p.latency ? FQ_NCLS : p.prefilter_first + 1); c++) launch(c, FIT_MAIN);   // (nearly all survivors are in the first of them)
    // the longest chains first.  (The one-wave class on the submission stream itself, so that it starts without the 60 .. 90 us
    // the fork event takes to reach a side stream -- measured with the wall clock inside the kernels -- cost 0.5 ms: its persistent
    // grid then holds the chip before the 128-thread class is placed, which ends up running last and alone.)
    // (holding the shorter-chained classes of a small submission back a few microseconds with a one-wave wait kernel ahead of
    // them, to get on plain streams -- a captured graph -- the placement order stream priorities give, measured nothing: 0.395 vs
    // 0.395 ms for one frame, 1.055 vs 1.065 for eight.  Priorities act on every slot that frees up, not on the first placement.)
    for (int c = p.prefilter_first - 1, a = 0; c >= 0; c--)
      if (launch(c, a < FQ_NAUX ? a : FQ_NAUX - 1)) a++;
  } else if ((uint64_t)n * (uint64_t)W * (uint64_t)H >= LARGE_FIRST_MIN_PX) {
    launch(FQ_C0 + 3, FIT_MAIN);
    launch(FQ_C0 + 4, FIT_MAIN);
    fork();   // both large classes are done
    // (which small class shares the chip with which was measured over seven assignments: 16.0 - 16.9 ms; best when the
    // 256-thread class is the one that ends up running last)
    for (int c = 0, a = 0; c <= FQ_C0 + 2; c++)
      if (launch(c, a % FQ_NAUX)) a++;
  } else {   // the longest chains side by side: the largest clusters | 4096..8192 then the one-wave class | the other two
    fork();
    launch(FQ_C0 + 4, FIT_MAIN);
    launch(FQ_C0 + 3, 0);
    launch(FQ_C0 + 2, 1);
    launch(FQ_C0 + 1, 2);
    launch(FQ_C0 + 0, 0);
    launch(0, 2);
  }

  unsigned gq = 2048u / n;
  p.decode_grid = gq < 96u ? 96u : (gq > 256u ? 256u : gq);   // about one wave per candidate quad of a noisy frame (16 per frame measured 0.36 ms slower)
  return p;
}

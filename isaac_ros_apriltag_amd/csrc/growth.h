// growth.h -- which capacity of a handle grows after a submission, and to what size; detector.hip reallocates (regrow).  Plain
// C++ without HIP, so that tests/test_growth_policy_cpu.py compiles it on the host; hence FrameCounters lives here too.
#pragma once
#include <stdint.h>

#include "../../include/apriltag_amd.h"   // AMDAT_FLAG_*

#define AT_FLAG_CANDS 0x20u   // internal frame flag: quad-candidate list full (never reported: grown, or reported as a quad overflow)

// Per-frame counters (one struct per batch slot), zeroed at the start of every submission.
struct FrameCounters {
  uint32_t npoints_raw;   // staged boundary points
  uint32_t nclusters;     // kept clusters
  uint32_t npoints_kept;  // points in kept clusters (allocation cursor)
  uint32_t nquads;
  uint32_t ndets;         // raw detections before reconcile
  uint32_t flags;         // AMDAT_FLAG_*
  uint32_t nout;          // detections after reconcile
  uint32_t nroots;        // tile-local component roots (CC root list)
  uint32_t ncand;         // quad candidates (four fitted lines) awaiting k_quad_finish
  uint32_t nlong;         // long staging records (k_points -> k_scatter)
  uint32_t seq;           // FrameDesc::seq of the launch that produced these counters, written last (k_reconcile): the host checks it
                          // after its stream wait, so results of an EARLIER launch can never be taken for this one's
};

// In the order plan_growth tries them.  GROW_POINTS: points, long records and pair table; GROW_HASH: plan_pending_hash.
enum GrowFamily : uint32_t { GROW_NONE = 0, GROW_CLUSTERS, GROW_QUADS, GROW_CANDS, GROW_POINTS, GROW_HASH };
// Per-frame capacities (DetParams' fields of the same names) and the long-record divisor: lcap = long_capacity(pcap, lcap_div).
struct GrowCaps { uint32_t pcap, lcap, hcap, ccap, qcap, cand_cap, lcap_div; };
// Hard limits, and which capacities follow the content (off once their growth failed).  The candidate list has no switch.
struct GrowLimits { uint32_t pcap_hard, hcap_hard, ccap_hard; bool points, hash, clusters, quads; };
struct GrowPlan {
  GrowFamily family;     // what to reallocate; GROW_NONE: the submission's results stand
  GrowCaps caps;         // the capacities after the growth
  bool cands_as_quads;   // a candidate overflow that does not grow: report it as AMDAT_FLAG_QUADS_OVERFLOW (report_cands_as_quads)
  bool hash_next;        // (GROW_NONE) the pair table is more than a quarter full: grow it before the next submission
};

inline uint32_t long_capacity(uint32_t pcap, uint32_t lcap_div) { return pcap / lcap_div > 4096u ? pcap / lcap_div : 4096u; }
inline uint32_t doubled(uint32_t cap, uint32_t limit) { return (uint64_t)cap * 2 > limit ? limit : cap * 2; }

// The next family to grow after a submission of n frames (one per relaunch), skipping those whose bit 1 << family is in `failed`.
inline GrowPlan plan_growth(const FrameCounters* fc, uint32_t n, const GrowCaps& c, const GrowLimits& lim, uint32_t failed = 0) {
  bool pts_over = false, long_over = false, hash_over = false, hash_crowded = false, quads_over = false, cands_over = false;
  uint32_t nlong_max = 0, ncl_max = 0;
  for (uint32_t f = 0; f < n; f++) {
    const FrameCounters& k = fc[f];
    // (the points flag covers the staging words and the long records: the counters, which count every attempt, say which it was)
    if (k.flags & AMDAT_FLAG_POINTS_OVERFLOW) {
      if (k.nlong > c.lcap) { long_over = true; if (k.nlong > nlong_max) nlong_max = k.nlong; }
      if (k.npoints_raw > c.pcap || k.nlong <= c.lcap) pts_over = true;
    }
    hash_over |= (k.flags & AMDAT_FLAG_HASH_OVERFLOW) != 0;
    hash_crowded |= k.nclusters > c.hcap / 4;
    if ((k.flags & AMDAT_FLAG_CLUSTERS_OVERFLOW) && k.nclusters > c.ccap && k.nclusters > ncl_max) ncl_max = k.nclusters;
    quads_over |= (k.flags & AMDAT_FLAG_QUADS_OVERFLOW) != 0 && k.nquads > c.qcap;
    cands_over |= (k.flags & AT_FLAG_CANDS) != 0;
  }
  GrowPlan g = {GROW_NONE, c, false, false};
  auto may = [&](GrowFamily f) { return (failed & (1u << f)) == 0; };
  if (ncl_max && lim.clusters && c.ccap < lim.ccap_hard && may(GROW_CLUSTERS)) {   // to the power of two that holds the fullest frame
    while (g.caps.ccap < ncl_max && g.caps.ccap < lim.ccap_hard) g.caps.ccap *= 2;
    if (g.caps.ccap > lim.ccap_hard) g.caps.ccap = lim.ccap_hard;
    g.family = GROW_CLUSTERS;
  } else if (quads_over && lim.quads && c.qcap < c.ccap && may(GROW_QUADS)) {
    g.caps.qcap = doubled(c.qcap, c.ccap);
    g.family = GROW_QUADS;
  } else if (cands_over && c.cand_cap < c.ccap && may(GROW_CANDS)) {   // (every kept cluster can become a candidate)
    g.caps.cand_cap = doubled(c.cand_cap, c.ccap);
    g.family = GROW_CANDS;
  } else {
    g.cands_as_quads = cands_over;
    const bool can_pts = lim.points && c.pcap < lim.pcap_hard, can_long = lim.points && c.lcap_div > 1;
    const bool can_hash = lim.hash && c.hcap < lim.hcap_hard;
    if (((pts_over && can_pts) || (long_over && can_long) || (hash_over && can_hash)) && may(GROW_POINTS)) {
      if (pts_over && can_pts) g.caps.pcap = doubled(c.pcap, lim.pcap_hard);
      if (long_over && can_long)   // the smallest share of the (new) point capacity that holds what this submission asked for
        do g.caps.lcap_div >>= 1; while (g.caps.lcap_div > 1 && g.caps.pcap / g.caps.lcap_div < nlong_max);
      g.caps.lcap = long_capacity(g.caps.pcap, g.caps.lcap_div);
      if (hash_over && can_hash) g.caps.hcap = doubled(c.hcap, lim.hcap_hard);
      g.family = GROW_POINTS;
    } else {
      g.hash_next = hash_crowded && can_hash;   // (not now: this submission's buffers may still be inspected)
    }
  }
  return g;
}

// The pair table of the last submission was crowded (GrowPlan::hash_next): its growth ahead of the next submission.
inline GrowPlan plan_pending_hash(const GrowCaps& c, const GrowLimits& lim) {
  GrowPlan g = {lim.hash && c.hcap < lim.hcap_hard ? GROW_HASH : GROW_NONE, c, false, false};
  if (g.family == GROW_HASH) g.caps.hcap = doubled(c.hcap, lim.hcap_hard);
  return g;
}

inline void give_up(GrowLimits& lim, GrowFamily f) {
  if (f == GROW_CLUSTERS) lim.clusters = false;
  if (f == GROW_QUADS) lim.quads = false;
  if (f == GROW_POINTS) lim.points = false;
  if (f == GROW_POINTS || f == GROW_HASH) lim.hash = false;
}

// Plans and applies growths until apply(plan) succeeds or none is left (GROW_NONE).  A family that failed is not picked again in
// the round: the candidate list, which has no switch to give up, would be.
template <class Apply>
inline GrowPlan grow_round(const FrameCounters* fc, uint32_t n, const GrowCaps& c, GrowLimits& lim, Apply&& apply) {
  GrowPlan g;
  for (uint32_t failed = 0;; failed |= 1u << g.family) {
    g = plan_growth(fc, n, c, lim, failed);
    if (g.family == GROW_NONE || apply(g)) return g;
    give_up(lim, g.family);
  }
}

// A candidate overflow that does not grow is, for the caller, what it amounts to: a quad-list overflow.
inline void report_cands_as_quads(FrameCounters* fc, uint32_t n) {
  for (uint32_t f = 0; f < n; f++)
    if (fc[f].flags & AT_FLAG_CANDS) fc[f].flags = (fc[f].flags & ~AT_FLAG_CANDS) | AMDAT_FLAG_QUADS_OVERFLOW;
}

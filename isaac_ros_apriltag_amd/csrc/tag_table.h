// tag_table.h -- the tag table of a handle (amdAprilTagsSetTagTable): which tags a deployment has and how
// big each one is.  Stated once, in plain C++, for host and device: tt_key and tt_lookup are __host__ __device__ under hipcc and
// ordinary inline functions under g++ (tests/aux_c/tag_table_driver.cpp compiles these lines and prints what they give;
// tests/tag_table_ref.py states them in Python).  k_reconcile, k_undistort_records and k_pose_refine look a record's size up here.
//
// The statement.  An entry is (family_index, id, size): family_index is the index into the handle's family list, id a tag id or
// AMDAT_TAG_ID_ANY (the largest admitted family has ids up to 65 534, so 0xFFFF is free as "every id of the family"), size the edge
// in metres held as (double)(float)size -- the way the handle's own tag_size reaches DetParams -- and 0 for "listed, at the handle's
// tag_size".  The key is family_index << 16 | id; the table is the keys in ascending order with the sizes beside them.  A record's
// size is the size of the entry with its exact key; failing that, of its family's wildcard entry; failing that, the default, and
// the record is not listed.  An exact entry therefore beats the wildcard, and at most 2 * 12 search steps answer (4096 entries).
#pragma once
#include <float.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TT_HD __host__ __device__ __forceinline__
#else
#define TT_HD static inline
#endif

#include "tools_hooks.h"   // TT_SEARCH_END, TT_WILDCARD_FIRST (the product build: n, false)

#ifndef AMDAT_MAX_TAG_ENTRIES
#define AMDAT_MAX_TAG_ENTRIES 4096u
#endif
#ifndef AMDAT_TAG_ID_ANY
#define AMDAT_TAG_ID_ANY 0xFFFFu
#endif
#define TT_MAX_FAMILIES 4u   // AT_MAX_FAMILIES: a family index takes the key's bits 16 and 17

// What device memory holds, in one buffer: the header, AMDAT_MAX_TAG_ENTRIES keys, AMDAT_MAX_TAG_ENTRIES sizes.  The kernels read
// count and flag from here, so new contents change no launch argument.
struct TagTableHeader {
  uint32_t n;             // entries
  uint32_t listed_only;   // 1: k_reconcile drops the records that are not listed
  uint32_t pad[2];
};
#define TT_KEYS_OFFSET 16u                                          // bytes: behind the header
#define TT_SIZES_OFFSET (TT_KEYS_OFFSET + 4u * AMDAT_MAX_TAG_ENTRIES)   // a multiple of 8
#define TT_BYTES (TT_SIZES_OFFSET + 8u * AMDAT_MAX_TAG_ENTRIES)

struct TagTableEntry {
  uint32_t family_index, id;
  float size;
};

TT_HD uint32_t tt_key(uint32_t family_index, uint32_t id) { return (family_index << 16) | id; }

// The position of `key` among keys[0 .. n), n if it is absent.
TT_HD uint32_t tt_find(const uint32_t* keys, uint32_t n, uint32_t key) {
  const uint32_t end = TT_SEARCH_END(n);   // (tools_hooks.h: n)
  uint32_t lo = 0, hi = end;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (keys[mid] < key) lo = mid + 1u; else hi = mid;
  }
  return (lo < end && keys[lo] == key) ? lo : n;
}

// The size of tag (family, id), and whether the table lists it.  A family or an id that no key can hold is not listed.
TT_HD double tt_lookup(const uint32_t* keys, const double* sizes, uint32_t n, uint32_t family, uint32_t id, double default_size,
                       bool* listed) {
  *listed = false;
  if (family >= TT_MAX_FAMILIES || id >= AMDAT_TAG_ID_ANY) return default_size;
  uint32_t at = TT_WILDCARD_FIRST ? n : tt_find(keys, n, tt_key(family, id));   // (tools_hooks.h: false)
  if (at == n) at = tt_find(keys, n, tt_key(family, AMDAT_TAG_ID_ANY));
  if (TT_WILDCARD_FIRST && at == n) at = tt_find(keys, n, tt_key(family, id));
  if (at == n) return default_size;
  *listed = true;
  const double s = sizes[at];
  return s == 0.0 ? default_size : s;
}

// The same on the buffer as device memory holds it; table == nullptr: no table, every tag is listed at the default.
TT_HD double tt_lookup_buf(const void* table, uint32_t family, uint32_t id, double default_size, bool* listed) {
  *listed = true;
  if (!table) return default_size;
  return tt_lookup((const uint32_t*)((const char*)table + TT_KEYS_OFFSET), (const double*)((const char*)table + TT_SIZES_OFFSET),
                   ((const TagTableHeader*)table)->n, family, id, default_size, listed);
}
TT_HD double tt_size_dev(const void* table, uint32_t family, uint32_t id, double default_size) {
  bool listed;
  return tt_lookup_buf(table, family, id, default_size, &listed);
}
TT_HD bool tt_listed_dev(const void* table, uint32_t family, uint32_t id) {
  bool listed;
  (void)tt_lookup_buf(table, family, id, 0.0, &listed);
  return listed;
}

// (host only) The sorted table of `entries` into keys[n], sizes[n].  0, or -1 where the table is refused: more than
// AMDAT_MAX_TAG_ENTRIES entries, a family index at or beyond num_families, an id at or beyond the family's code count other than
// the wildcard, a negative or non-finite size, two entries with one key.  keys and sizes are the caller's scratch: where the table
// is refused they hold nothing of use.
static inline int tt_build(uint32_t num_families, const uint32_t* ncodes, uint32_t n, const TagTableEntry* entries, uint32_t* keys,
                           double* sizes) {
  if (n > AMDAT_MAX_TAG_ENTRIES || num_families > TT_MAX_FAMILIES || (n && !entries)) return -1;
  for (uint32_t i = 0; i < n; i++) {
    const TagTableEntry& e = entries[i];
    if (e.family_index >= num_families || e.id > AMDAT_TAG_ID_ANY) return -1;
    if (e.id != AMDAT_TAG_ID_ANY && e.id >= ncodes[e.family_index]) return -1;
    if (!(e.size >= 0.0f && e.size <= FLT_MAX)) return -1;   // (negative, infinite, or a NaN, which fails every comparison)
    // insertion into the sorted prefix (at most 4096 entries, once per setter call)
    const uint32_t key = tt_key(e.family_index, e.id);
    uint32_t j = i;
    while (j > 0 && keys[j - 1] > key) { keys[j] = keys[j - 1]; sizes[j] = sizes[j - 1]; j--; }
    if (j > 0 && keys[j - 1] == key) return -1;
    keys[j] = key;
    sizes[j] = (double)e.size;
  }
  return 0;
}

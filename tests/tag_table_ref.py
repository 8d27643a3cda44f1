"""The tag table (csrc/tag_table.h) stated in plain Python: an entry is (family_index, id, size); the key is
family_index << 16 | id; a tag's size is that of the entry with its exact key, failing that of its family's wildcard entry, failing
that the default, and then the tag is not listed.  Sizes are held as the double of the float the C ABI carries; 0 stands for the
default.  No sorting and no search here: a dictionary says the same thing."""
import math

import numpy as np

MAX_ENTRIES = 4096
ID_ANY = 0xFFFF
MAX_FAMILIES = 4


def f32(v):
    return float(np.float32(v))


def key(family_index, tag_id):
    return (family_index << 16) | tag_id


def build(num_families, ncodes, entries):
    """{key: size} of entries = [(family_index, id, size)], or None where the table is refused: more than MAX_ENTRIES entries, a family
    index at or beyond num_families, an id at or beyond the family's code count other than the wildcard, a negative or non-finite
    size, two entries with one key."""
    if len(entries) > MAX_ENTRIES:
        return None
    table = {}
    for fi, tid, size in entries:
        if fi >= num_families or (tid != ID_ANY and tid >= ncodes[fi]):
            return None
        s = float(np.float32(size))
        if not math.isfinite(s) or s < 0.0:
            return None
        if key(fi, tid) in table:
            return None
        table[key(fi, tid)] = s
    return table


def lookup(table, family, tag_id, default_size, wildcard_first=False):
    """(size, listed) of tag (family, id).  wildcard_first: the form of wrong build 54."""
    if family >= MAX_FAMILIES or tag_id >= ID_ANY:
        return default_size, False
    order = (key(family, ID_ANY), key(family, tag_id)) if wildcard_first else (key(family, tag_id), key(family, ID_ANY))
    for k in order:
        if k in table:
            return (table[k] if table[k] != 0.0 else default_size), True
    return default_size, False


def lookup_without_last(table, family, tag_id, default_size):
    """The form of wrong build 53: the entry with the largest key is never found."""
    cut = dict(table)
    if cut:
        del cut[max(cut)]
    return lookup(cut, family, tag_id, default_size)


def filter_listed(table, records, family_index=lambda r: r["family"]):
    """The records the listed-only table keeps, in order."""
    return [r for r in records if lookup(table, family_index(r), int(r["id"]), 0.0)[1]]

// orlg_inst.h -- what the instantiation units (orlg_inst_*.hip) repeat: each is compiled for ONE word count, -DORLG_INST_W=<W>, one
// object per W so that the library builds in parallel (build.py), and exports its lookups under names that end in that W.  Which
// keys a unit holds: orlg_variants.h.
#pragma once
#include "orlg_variants.h"

#ifndef ORLG_INST_W
#error "compile with -DORLG_INST_W=<words per link>"
#endif
#define ORLG_CAT2(a, b) a##b
#define ORLG_CAT(a, b) ORLG_CAT2(a, b)

// the unit's lookup `lookup`<W>(Key): the instantiation of every key of KEYS (a list, or a unit's lists, of orlg_variants.h) in the
// list's order -- the order of the kernels in the code object -- and null for any other key.  ENTRY: the family's ORLG_INST_* below
#define ORLG_INST_LOOKUP(type, lookup, Key, KEYS, ENTRY)  \
    type ORLG_CAT(lookup, ORLG_INST_W)(Key key) {         \
        KEYS(ENTRY)                                       \
        return nullptr;                                   \
    }
#define ORLG_INST_WAVE(name, ...) if (key == OrlgWaveKey{ORLG_WAVE_KERNEL(name), __VA_ARGS__}) return name<ORLG_INST_W, __VA_ARGS__>;
#define ORLG_INST_MM(...) if (key == OrlgMmKey{__VA_ARGS__}) return orlg_rmsa_mm_kernel<ORLG_INST_W, __VA_ARGS__>;
#define ORLG_INST_AM(...) if (key == OrlgAmKey{__VA_ARGS__}) return orlg_rmsa_am_kernel<ORLG_INST_W, __VA_ARGS__>;
#define ORLG_INST_GROUP(...) if (key == OrlgGroupKey{__VA_ARGS__}) return orlg_rmsa_group_kernel<ORLG_INST_W, __VA_ARGS__>;
#define ORLG_INST_PHY(...) if (key == OrlgPhyKey{__VA_ARGS__}) return orlg_phy_kernel<ORLG_INST_W, __VA_ARGS__>;
// the lookup of a single kernel (a row of ORLG_WAVE_QUERIES)
#define ORLG_INST_QUERY(type, lookup, kernel) type ORLG_CAT(lookup, ORLG_INST_W)() { return kernel<ORLG_INST_W>; }

// Host build of panda_amd/csrc/xcd_remap.h: the scatter kernels of the bucket sort take their tile from this very function, so a map
// that is not a bijection would sort a tile twice and another one never.  tests/test_msm_tail_shapes.py checks it for every grid size.
#include "../../panda_amd/csrc/xcd_remap.h"

extern "C" unsigned xcd_remap_host(unsigned id, unsigned nwg) { return panda::xcd_remap(id, nwg); }

// 0 if id -> xcd_remap(id, nwg) is a bijection of [0, nwg) under which the ids of one class (id mod 8, in ascending order) take
// consecutive tiles; otherwise 1 + the first id at fault.  `seen` has room for nwg bytes.
extern "C" unsigned xcd_remap_check(unsigned nwg, unsigned char *seen)
{
    for (unsigned i = 0; i < nwg; i++) seen[i] = 0;
    for (unsigned id = 0; id < nwg; id++) {
        const unsigned t = panda::xcd_remap(id, nwg);
        if (t >= nwg || seen[t]) return 1 + id;
        seen[t] = 1;
        if (id >= panda::XCDS && t != panda::xcd_remap(id - panda::XCDS, nwg) + 1) return 1 + id;
    }
    return 0;
}

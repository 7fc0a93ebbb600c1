// The lock-free union-find of the labelling kernels (sgm_speckle.hip,
// mesh_clean.hip) over an array of 32-bit labels, label[i] == i at the start.
// Invariant of every store: a parent's index is never larger than the
// element's own and a label only ever decreases (fetch_min), so every find
// loop ends at an element that is its own parent, whatever it read on the way,
// and no thread waits for another.
#pragma once

#include "common.h"

namespace smvs_hip {

// SCOPE: __HIP_MEMORY_SCOPE_WORKGROUP for labels in LDS,
// __HIP_MEMORY_SCOPE_AGENT for global labels (the L2 caches of the XCDs are
// not coherent with each other for plain loads)
template <int SCOPE>
__device__ __forceinline__ uint32_t
uf_find(uint32_t *label, uint32_t a)
{
    uint32_t p = __hip_atomic_load(label + a, __ATOMIC_RELAXED, SCOPE);
    while (p != a) {   // p < a
        a = p;
        p = __hip_atomic_load(label + a, __ATOMIC_RELAXED, SCOPE);
    }
    return a;
}

// The larger root gets the smaller one as its parent.  Where another thread
// lowered label[a] first, `old` is below a and the loop goes on from there:
// max(a, b) falls with every pass.
template <int SCOPE>
__device__ __forceinline__ void
uf_union(uint32_t *label, uint32_t a, uint32_t b)
{
    for (;;) {
        a = uf_find<SCOPE>(label, a);
        b = uf_find<SCOPE>(label, b);
        if (a == b)
            return;
        if (a < b) {
            uint32_t const t = a;
            a = b;
            b = t;
        }
        uint32_t const old = __hip_atomic_fetch_min(label + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a)
            return;
        a = old;
    }
}

} // namespace smvs_hip

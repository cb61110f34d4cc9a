// What the two promotion launches share - ga_promote_kernel (offspring.hip, fp32 slabs) and ga16_promote_kernel
// (fc16_offspring.hip, fp16 slabs): the limits of their compile-time recursions, the selection of a workgroup's role from
// the by-value kernel argument and the host-side check of the roles.  The recursions themselves stay beside their kernels:
// one addresses float* + net * stride + s0, the other uint4* + net * pitch, and ga_promote_kernel keeps its register
// figures only in its own form (profiles/r13_breeding_helpers.md).
#pragma once
#include "coevo_common.hip.h"

namespace coevo {

constexpr int PROMOTE_MAX_E = 8, PROMOTE_MAX_HOF = 16;

// coevo_ga_promote_role and coevo_ga16_promote_role are one layout, with typed and with untyped regions
static_assert(sizeof(coevo_ga_promote_role) == 48 && sizeof(coevo_ga16_promote_role) == 48,
              "layout mirrored by coevonet_amd/lib.py GaPromoteRole");

struct PromoteRole {
    void *pop, *hof, *elite;
    const int32_t *order;
    int D, from_pop, to_pop0;
};

// role y of a by-value kernel argument `a` that holds `role[3]`: field-wise scalar selects (indexing the argument array
// dynamically copies it to scratch, and so does handing `a` to a function by reference - hence a macro)
#define PROMOTE_SEL(a, y, f) ((y) == 0 ? (a).role[0].f : ((y) == 1 ? (a).role[1].f : (a).role[2].f))
#define PROMOTE_ROLE(a, y)                                                                                          \
    PromoteRole{PROMOTE_SEL(a, y, pop), PROMOTE_SEL(a, y, hof), PROMOTE_SEL(a, y, elite), PROMOTE_SEL(a, y, order), \
                PROMOTE_SEL(a, y, D), PROMOTE_SEL(a, y, elites_from_pop), PROMOTE_SEL(a, y, best_to_pop0)}

// host side: the roles of a promotion launch checked and copied into the kernel's argument; false = a bad argument
template <class Args, class Role>
static inline bool promote_roles(Args &a, const Role *roles, int n_roles, int E, int hof, bool need_aligned16)
{
    if (!roles || n_roles < 1 || n_roles > 3 || E < 1 || E > PROMOTE_MAX_E || hof < 1 || hof > PROMOTE_MAX_HOF) return false;
    for (int r = 0; r < n_roles; ++r) {
        const Role &R = roles[r];
        if (!R.pop || !R.hof || !R.elite || !fc_dim_ok(R.D) || (R.elites_from_pop && !R.order)) return false;
        if (need_aligned16 && !(aligned16(R.pop) && aligned16(R.hof) && aligned16(R.elite))) return false;
        a.role[r] = R;
    }
    a.E = E; a.hof = hof;
    return true;
}

}  // namespace coevo

// LDS layout of the generic feature kernel (adh_features.hip) and the launch groups of its class.
// Shared with the plan (adh_plan.hip), which sizes every generic candidate by its OWN layout.
#pragma once
#include "adh_device.h"

namespace feat {

// LDS regions.  Element counts depend only on the capacities: a candidate's own (fragments kept, observations,
// cycles, isotopes).  `spill`: the three [K][O][F] planes fi, fm, ffp and bp[K][F] are NOT in LDS but in the
// candidate's spill block in the scratch slab (spill_bytes); everything indexed by K, K*O, O, I or F alone stays.
struct Layout {
    int Kc, Oc, Fc, Ic;
    bool spill;
    __host__ __device__ Layout(const Caps &c, bool spill_ = false) : Kc(c.k), Oc(c.o), Fc(c.f), Ic(c.i), spill(spill_) {}
    // doubles
    __host__ __device__ int d_wt() const { return 0; }
    __host__ __device__ int d_wtp() const { return d_wt() + Oc * 2 * Fc; }
    __host__ __device__ int d_qtf() const { return d_wtp() + 2 * Fc; }
    __host__ __device__ int d_omz() const { return d_qtf() + Ic * Oc; }
    __host__ __device__ int d_ohe() const { return d_omz() + Kc * Oc; }
    __host__ __device__ int d_pk() const { return d_ohe() + Kc * Oc; }   // [4][Kc]: mzmean,height,area,merr
    __host__ __device__ int d_po() const { return d_pk() + 4 * Kc; }     // [2][Oc]: esc, efc
    __host__ __device__ int d_pi() const { return d_po() + 2 * Oc; }     // [2][Ic]: hp, omzp
    __host__ __device__ int n_double() const { return d_pi() + 2 * Ic; }
    // floats (after the doubles)
    __host__ __device__ int f_tile() const { return 0; }                 // [3][Kc*Oc*Fc]: fi, fm, ffp (not when spilled)
    __host__ __device__ int f_prec() const { return f_tile() + (spill ? 0 : 3 * Kc * Oc * Fc); }  // [2][Ic*Fc]
    __host__ __device__ int f_tpl() const { return f_prec() + 2 * Ic * Fc; }        // [2][Oc*Fc]
    __host__ __device__ int f_bp() const { return f_tpl() + 2 * Oc * Fc; }          // [Kc*Fc] (not when spilled)
    __host__ __device__ int f_pk() const { return f_bp() + (spill ? 0 : Kc * Fc); } // [6][Kc]
    __host__ __device__ int f_pko() const { return f_pk() + 6 * Kc; }    // [3][Kc*Oc]
    __host__ __device__ int f_po() const { return f_pko() + 3 * Kc * Oc; }  // [4][Oc]
    __host__ __device__ int f_pi() const { return f_po() + 4 * Oc; }     // [3][Ic]
    __host__ __device__ int f_pf() const { return f_pi() + 3 * Ic; }     // [3][Fc]
    __host__ __device__ int f_feat() const { return f_pf() + 3 * Fc; }
    __host__ __device__ int n_float() const { return f_feat() + ADH_NUM_FEATURES; }
    // ints (after the floats)
    __host__ __device__ int i_pk() const { return 0; }                   // [3][Kc]: present, kmap, ord
    __host__ __device__ int i_pko() const { return i_pk() + 3 * Kc; }    // [Kc*Oc]: fpeak
    __host__ __device__ int i_obs() const { return i_pko() + Kc * Oc; }  // [Oc]
    __host__ __device__ int n_int() const { return i_obs() + Oc; }
    // bytes (after the ints): [5][Kc]
    __host__ __device__ int n_byte() const { return ((5 * Kc + 7) / 8) * 8; }
    __host__ __device__ size_t bytes() const {
        size_t b = (size_t)n_double() * 8;
        b += ((size_t)n_float() * 4 + 7) / 8 * 8;
        b += ((size_t)n_int() * 4 + 7) / 8 * 8;
        b += n_byte();
        return b;
    }
};

// a generic candidate's own capacities (the plan and the kernel must agree on them).  An axis of length 0 gives
// regions of no bytes: such a candidate keeps no fragment and leaves the kernel before it indexes one.
__host__ __device__ inline Caps own_caps(uint32_t k_cap, int O, int F, int I) {
    Caps c{};
    c.k = (int32_t)k_cap;
    c.o = O;
    c.f = F;
    c.i = I;
    return c;
}

// the spill block of a candidate, behind its gather cells in the scratch slab: fi, fm, ffp [K][O][F] and bp [K][F]
__host__ __device__ inline uint64_t spill_bytes(const Caps &c) {
    const uint64_t n = 3ull * (uint64_t)c.k * c.o * c.f + (uint64_t)c.k * c.f;
    return (n * 4 + 31) / 32 * 32;
}

// own layout bytes with the sums in 64 bits, saturated: a slice of a million fragments must not wrap into a small tile
__host__ __device__ inline uint32_t own_layout_bytes(const Caps &c, bool spill) {
    const uint64_t k = c.k, o = c.o, f = c.f, i = c.i;
    const uint64_t cells = (spill ? 0 : 3 * k * o * f + k * f) * 4;
    const uint64_t rest = 48 * k * o + 80 * k + 64 * o * f + 64 * i * f + 64 * (o + i + f) + 1024;  // above every other region
    if (cells + rest >= (1ull << 31)) return 0x7FFFFFFFu;
    return (uint32_t)Layout(c, spill).bytes();
}

}  // namespace feat

// Launch groups of the generic class (internal to class 36; adh_plan_class_counts reports their sum):
//   0  own layout up to ADH_GENERIC_SMALL_LDS: several blocks of a launch share a CU
//   1  own layout up to ADH_GENERIC_LDS_LIMIT: one block per CU
//   2  own layout beyond it: the spill instantiation, bounded by its own (smaller) layout
// The kernel's static LDS (gram / redm of the MFMA contraction, 2 x 16 x 17 floats) comes on top of the dynamic block.
#define ADH_GENERIC_GROUPS 3
#define ADH_GENERIC_GROUP_SPILL 2
#define ADH_FEATURE_STATIC_LDS (2 * 16 * 17 * 4)
#define ADH_GENERIC_LDS_LIMIT (160 * 1024 - ADH_FEATURE_STATIC_LDS)
#define ADH_GENERIC_SMALL_LDS (40 * 1024 - ADH_FEATURE_STATIC_LDS)

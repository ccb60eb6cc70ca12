// LDS layout of the ion-mobility feature kernel (adh_features_im.hip) and the launch groups of its dynamic route.
// Shared with the plan (adh_plan.hip), which sizes every candidate by its OWN dynamic layout.
#pragma once
#include "adh_device.h"

// plan class of one-observation candidates with a small tile (adh_plan.hip), and what the plan admits to it
#define ADH_CLASS_IM_SMALL 2
#define ADH_IM_SMALL_K 12
#define ADH_IM_SMALL_S 32
#define ADH_IM_SMALL_F 24
#define ADH_IM_SMALL_SF 640

namespace featim {

// LDS capacities of a launch: taken from the launch's Caps (DimsDyn) or fixed at compile time (DimsFix), which
// turns every array address below into an instruction offset - with run-time capacities the ~60 array bases
// are scalar registers, more than there are, and the kernel spends a sixth of its instructions moving
// them between scalar registers and the lanes of spill registers
struct DimsDyn {
    int Kc, Oc, Sc, Fc, Ic, SFc;  // SFc: cells of one (scan, cycle) plane
    __host__ __device__ DimsDyn(const Caps &c) : Kc(c.k), Oc(c.o), Sc(c.s), Fc(c.f), Ic(c.i), SFc(c.s * c.f) {}
};
template <int K, int O, int S, int F, int I, int SF>
struct DimsFix {
    static constexpr int Kc = K, Oc = O, Sc = S, Fc = F, Ic = I, SFc = SF;
    __host__ __device__ DimsFix(const Caps &) {}
    __host__ __device__ static bool holds(const Caps &c) { return holds_axes(c) && c.s * c.f <= SF; }
    // (without the plane size: for a launch whose candidates were admitted one by one, plan class ADH_CLASS_IM_SMALL)
    __host__ __device__ static bool holds_axes(const Caps &c) {
        return c.k <= K && c.o <= O && c.s <= S && c.f <= F && c.i <= I;
    }
};
// SP (the spill instantiation of a candidate whose own layout exceeds the LDS of a CU): the float regions that grow with
// K * O * (S + F) - the work region and the profiles of R1 and R2 - are NOT in LDS but in the candidate's spill block
// in the scratch slab (featim::spill_bytes); R1 keeps the template, everything indexed by K * O, K, O * S * F or less stays.
template <class D, bool SP = false>
struct LayoutT : D {
    static constexpr bool spilled = SP;
    __host__ __device__ LayoutT(const Caps &c) : D(c) {}
    // doubles
    // (the transfer function is dead after the template; the per-fragment results and the frame times,
    // born later, take its place)
    __host__ __device__ int d_qtf() const { return 0; }                      // [Ic][Oc][Sc], early
    __host__ __device__ int qtf_size() const {
        const int a = D::Ic * D::Oc * D::Sc, b = 4 * D::Kc + D::Fc;
        return a > b ? a : b;
    }
    __host__ __device__ int d_pk() const { return d_qtf(); }                 // [4][Kc], late
    __host__ __device__ int d_frt() const { return d_qtf() + 4 * D::Kc; }       // [Fc] frame rt (float64), late
    __host__ __device__ int d_omz() const { return d_qtf() + qtf_size(); }
    __host__ __device__ int d_ohe() const { return d_omz() + D::Kc * D::Oc; }
    __host__ __device__ int d_omzu() const { return d_ohe() + D::Kc * D::Oc; }  // per selected fragment,
    __host__ __device__ int d_oheu() const { return d_omzu() + D::Kc * D::Oc; } // before the presence mask
    __host__ __device__ int d_accw() const { return d_oheu() + D::Kc * D::Oc; } // [2][Kc*Oc] weight sums
    __host__ __device__ int d_po() const { return d_accw() + 2 * D::Kc * D::Oc; }   // [2][Oc]
    __host__ __device__ int d_pi() const { return d_po() + 2 * D::Oc; }     // [2][Ic]
    __host__ __device__ int n_double() const { return d_pi() + 2 * D::Ic; }
    // floats
    __host__ __device__ int smax() const { return D::Sc > D::Fc ? D::Sc : D::Fc; }
    __host__ __device__ int f_wb() const { return 0; }                            // work [Kc*Oc*max(Sc,Fc)]
    // Two regions are used twice.  R1 holds the template until its profiles are taken, then the masked
    // frame / scan profiles; R2 holds the profiles before the presence mask, then the scan envelopes and
    // the quantification profiles.  (LDS per block is what bounds the resident waves of this kernel, and
    // the kernel's time follows them: 26 KB -> 40 KB per block costs 38 %.)
    // (the work region also takes the isotope scan sums [Ic][Sc] of a materialised tile: larger only where Kc * Oc < Ic)
    __host__ __device__ int work_size() const {
        const int a = D::Kc * D::Oc * smax(), b = D::Ic * D::Sc;
        return a > b ? a : b;
    }
    __host__ __device__ int prof_size() const { return D::Kc * D::Oc * (D::Fc + D::Sc); }  // profiles of R1 (late) / R2
    __host__ __device__ int f_work_end() const { return f_wb() + (SP ? 0 : work_size()); }
    __host__ __device__ int r1_size() const {
        const int a = D::Oc * D::SFc, b = SP ? 0 : prof_size();
        return a > b ? a : b;
    }
    __host__ __device__ int f_r1() const { return f_work_end(); }
    __host__ __device__ int f_r2() const { return f_r1() + r1_size(); }
    __host__ __device__ int f_tpl() const { return f_r1(); }                      // [Oc*Sc*Fc]       R1, early
    __host__ __device__ int f_ffp() const { return f_r1(); }                      // [Kc*Oc*Fc]       R1, late
    __host__ __device__ int f_fspr() const { return f_r1() + D::Kc * D::Oc * D::Fc; }      // [Kc*Oc*Sc] raw   R1, late
    __host__ __device__ int f_ffpu() const { return f_r2(); }                     // [Kc*Oc*Fc] before the mask  R2, early
    __host__ __device__ int f_fspu() const { return f_r2() + D::Kc * D::Oc * D::Fc; }      // [Kc*Oc*Sc] before the mask  R2, early
    __host__ __device__ int f_fspe() const { return f_r2(); }                     // [Kc*Oc*Sc] envelope  R2, late
    __host__ __device__ int f_bp() const { return f_r2() + D::Kc * D::Oc * D::Sc; }        // [Kc*Fc]          R2, late
    __host__ __device__ int f_tfp() const { return f_r2() + (SP ? 0 : prof_size()); }  // [Oc*Fc]
    __host__ __device__ int f_tsp() const { return f_tfp() + 2 * D::Oc * D::Fc; }       // [2][Oc*Sc] (tfp: raw, env)
    __host__ __device__ int f_qm() const { return f_tsp() + 2 * D::Oc * D::Sc; }        // [Oc*Sc] qtf mask
    __host__ __device__ int f_pk() const { return f_qm() + D::Oc * D::Sc; }             // [8][Kc]
    __host__ __device__ int f_pko() const { return f_pk() + 8 * D::Kc; }             // [4][Kc*Oc]
    __host__ __device__ int f_po() const { return f_pko() + 4 * D::Kc * D::Oc; }        // [4][Oc]
    __host__ __device__ int f_pi() const { return f_po() + 4 * D::Oc; }              // [3][Ic]
    __host__ __device__ int f_pf() const { return f_pi() + 3 * D::Ic; }              // [2][Fc]
    __host__ __device__ int f_feat() const { return f_pf() + 2 * D::Fc; }
    __host__ __device__ int n_float() const { return f_feat() + ADH_NUM_FEATURES; }
    // ints
    __host__ __device__ int i_pk() const { return 0; }                   // [4][Kc]
    __host__ __device__ int i_pko() const { return i_pk() + 4 * D::Kc; }    // [Kc*Oc]
    __host__ __device__ int i_obs() const { return i_pko() + D::Kc * D::Oc; }  // [Oc]
    __host__ __device__ int n_int() const { return i_obs() + D::Oc; }
    __host__ __device__ int n_byte() const { return ((5 * D::Kc + 7) / 8) * 8; }
    __host__ __device__ size_t bytes() const {
        size_t b = (size_t)n_double() * 8;
        b += ((size_t)n_float() * 4 + 7) / 8 * 8;
        b += ((size_t)n_int() * 4 + 7) / 8 * 8;
        b += n_byte();
        return b;
    }
};
using Layout = LayoutT<DimsDyn>;
using LayoutSpill = LayoutT<DimsDyn, true>;
// the common shape: up to 12 fragments, one observation, 40 scans, 32 cycles, 1152 cells per plane, 3 isotopes
// (13 704 + 2 560 static bytes: ten blocks per CU, as the specified 38 x 29 tiles get with run-time capacities)
using DimsCommon = DimsFix<12, 1, 40, 32, 3, 1152>;
using LayoutCommon = LayoutT<DimsCommon>;
// the same shape with two observations (plan class 1; only the tile part of the split path uses it)
using DimsCommon2 = DimsFix<12, 2, 40, 32, 3, 1152>;
using LayoutCommon2 = LayoutT<DimsCommon2>;
// small tiles (plan class ADH_CLASS_IM_SMALL): 10 248 + 2 560 bytes, twelve blocks per CU
using DimsSmall = DimsFix<ADH_IM_SMALL_K, 1, ADH_IM_SMALL_S, ADH_IM_SMALL_F, 3, ADH_IM_SMALL_SF>;
using LayoutSmall = LayoutT<DimsSmall>;

// a candidate's own capacities on the dynamic route (the plan and the kernel must agree on them): the fragments it may
// keep, its observations (one in the one-observation classes, whose candidates may have none and keep nothing then),
// its scans, cycles and the isotopes of the call (at least one).  An axis of length 0 gives regions of no bytes: such a candidate keeps
// no fragment and leaves the kernel before it indexes one.
__host__ __device__ inline Caps own_caps(uint32_t k_cap, int n_obs, int S, int F, int I) {
    Caps c{};
    c.k = (int32_t)k_cap;
    c.o = n_obs > 1 ? n_obs : 1;
    c.s = S;
    c.f = F;
    c.i = I > 1 ? I : 1;  // (top_k_isotopes = 0: one, as in the launch-wide Caps of the fixed layouts)
    return c;
}

// the spill block of a candidate, behind its gather cells in the scratch slab: the work region, then the profiles of
// R1 (ffp, fsp_raw) and of R2 (ffp_u, fsp_u; later fsp, bp), laid out as in LDS
__host__ __device__ inline uint64_t spill_floats(const Caps &c) {
    const uint64_t k = c.k, o = c.o, s = c.s, f = c.f, i = c.i;
    const uint64_t work = k * o * (s > f ? s : f), iso = i * s;
    return (work > iso ? work : iso) + 2 * k * o * (f + s);
}
__host__ __device__ inline uint64_t spill_bytes(const Caps &c) { return (spill_floats(c) * 4 + 31) / 32 * 32; }

// own layout bytes with the sums in 64 bits, saturated: a slice of a million fragments must not wrap into a small tile
__host__ __device__ inline uint32_t own_layout_bytes(const Caps &c, bool spill) {
    // (axes below 2^11 with at most 8 observations stay below 2^31 bytes in the layout's own 32-bit sums - 3 * 2^11 * 8 *
    // 2^12 floats at the most: nearly every candidate, and the plan kernel is spared some 150 instructions of 64-bit sums)
    const bool small_axes = ((uint32_t)c.k | (uint32_t)c.s | (uint32_t)c.f) < 2048u && (uint32_t)c.o <= 8u && (uint32_t)c.i <= 64u;
    if (!small_axes) {
        const uint64_t k = c.k, o = c.o, s = c.s, f = c.f, i = c.i;
        const uint64_t cells = (spill ? 0 : spill_floats(c)) * 4 + o * s * f * 4;
        const uint64_t rest = 8 * i * o * s + 128 * k * o + 128 * k + 32 * o * (s + f) + 16 * f + 64 * (o + i) + 1024;  // above every other region
        if (cells + rest >= (1ull << 31)) return 0x7FFFFFFFu;
    }
    return (uint32_t)(spill ? LayoutSpill(c).bytes() : Layout(c).bytes());
}

}  // namespace featim

#define ADH_IM_STAGE 128          // cells staged per round of the tile passes (two per lane)
#define ADH_IM_STATIC_LDS (ADH_IM_STAGE * 20)  // static LDS of adh_feature_im_kernel (chunk lists / Gram matrices: 2 176 B)

// Launch groups of the dynamic route (inside a plan class; adh_plan_class_counts reports the class):
//   0  own layout up to ADH_GENERIC_SMALL_LDS: several blocks of a launch share a CU (the edge is the generic kernel's,
//      and as untuned here as there)
//   1  own layout up to ADH_IM_LDS_LIMIT: one block per CU
//   2  own layout beyond it: the spill instantiation, bounded by its own (smaller) layout
// A class whose launch takes a fixed layout holds candidates of group 0 only (DimsCommon2 at its capacities: 30 KB).
#define ADH_IM_GROUPS 3
#define ADH_IM_GROUP_SPILL 2
#define ADH_IM_LDS_LIMIT (160 * 1024 - ADH_IM_STATIC_LDS)
// plan classes of an ion-mobility plan, in processing order, as slots of the per-class tables: 0, 1, ADH_CLASS_IM_SMALL, generic
#define ADH_IM_CLASS_SLOTS 4

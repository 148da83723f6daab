// bcf_cell.hpp -- one sample's FORMAT values of a BCF record -> the sample table's values (uz_types.h: uz_samples_view): genotype code, ref / alt
// depth and floor(GQ) in the 16-bit encoding, OR "unsettled".  __host__ __device__: k_bcf_cells (k_bcf.hip) and tests/bcf_cell_main.cpp run this
// very body.
//
// A field arrives as (pointer to THIS sample's values, descriptor); the descriptor is uz_vcf_bcf_view's: BCF type in the low four bits, values per
// sample above, 0 = the record has no such field.  A settled cell equals what the host's reader (io_vcf.cpp: bcf_sample_cell) and the pack rules
// (uz_samples_pack) make of the same bytes; whatever the 16-bit rows cannot hold is unsettled and goes back to the host (uz_samples_settle):
//   GT       the first two entries up to end-of-vector; allele = (x >> 1) - 1, below 0 (x of 0 or 1, the missing marker, a negative x) = missing;
//            one entry = haploid, half-missing calls count with their called allele
//   depths   AD's first two entries (one entry, or end-of-vector in the second: alt missing); a missing first entry with end-of-vector (or nothing)
//            behind it -- the text form's bare "." -- falls through to RO / AO when the record has both.  Missing / end-of-vector -> 0xFFFF,
//            0 .. 32767 the value; above 32767 (the wide list is the host's business) and below 0 (the pack's -1 or its ValueError): unsettled
//   GQ       integer types: missing, end-of-vector or below 0 -> 0xFFFF, else min(x, 32767).  Float: the two reserved bit patterns -> 0xFFFF,
//            else floorf (exact) -- NaN and anything below 0 -> 0xFFFF, above 32767 -> 32767
//   types    int8 / int16 / int32 (and float for GQ); any other type: unsettled (the host marks such records itself and never sends them)
// Replaces, for the cells it settles, cyvcf2's gt_types / gt_ref_depths / gt_alt_depths / gt_quals (informative_site_finder.py:257-260) on a .bcf
// (:41-43, :213).
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "vcf_cell.hpp"

#define UZ_BC_INT8 1u
#define UZ_BC_INT16 2u
#define UZ_BC_INT32 3u
#define UZ_BC_FLOAT 5u

#define UZ_BC_OK 0
#define UZ_BC_MISSING 1
#define UZ_BC_EOV 2

// bytes of one value of a type (0: a type without values, or none this body reads)
UZ_VC_HD uint32_t uz_bc_size(uint32_t type) { return type == UZ_BC_INT8 ? 1u : type == UZ_BC_INT16 ? 2u : (type == UZ_BC_INT32 || type == UZ_BC_FLOAT) ? 4u : 0u; }

UZ_VC_HD int32_t uz_bc_load16(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const int16_t *>(p); // (a field's array starts on a 4-byte boundary of the chunk's image)
#else
    int16_t x;
    memcpy(&x, p, 2);
    return x;
#endif
}
UZ_VC_HD uint32_t uz_bc_load32(const uint8_t *p) {
#if defined(__HIP_DEVICE_COMPILE__)
    return *reinterpret_cast<const uint32_t *>(p);
#else
    uint32_t x;
    memcpy(&x, p, 4);
    return x;
#endif
}

// k-th entry of an integer vector: a value, the missing marker or end-of-vector (type: UZ_BC_INT8 / 16 / 32)
UZ_VC_HD int uz_bc_int(uint32_t type, const uint8_t *p, uint32_t k, int32_t &out) {
    int32_t x, lowest;
    if (type == UZ_BC_INT8) { x = (int8_t)p[k]; lowest = -128; }
    else if (type == UZ_BC_INT16) { x = uz_bc_load16(p + 2 * k); lowest = -32768; }
    else { x = (int32_t)uz_bc_load32(p + 4 * k); lowest = INT32_MIN; }
    if (x == lowest) return UZ_BC_MISSING;
    if (x == lowest + 1) return UZ_BC_EOV;
    out = x;
    return UZ_BC_OK;
}

UZ_VC_HD bool uz_bc_is_int(uint32_t type) { return type == UZ_BC_INT8 || type == UZ_BC_INT16 || type == UZ_BC_INT32; }

// one depth: status + value -> the 16-bit encoding, or not settled (-> false)
UZ_VC_HD bool uz_bc_depth(int st, int32_t x, uint32_t &out) {
    if (st != UZ_BC_OK) { out = UZ_VC_MISSING; return true; }
    if (x < 0 || x > (int32_t)UZ_VC_MAX) return false;
    out = (uint32_t)x;
    return true;
}

// The cell of one sample: *_p points at this sample's values of the field, *_d is the field's descriptor (0: absent; then the pointer is not read).
UZ_VC_HD UzVcfCell uz_bcf_cell(const uint8_t *gt_p, uint32_t gt_d, const uint8_t *ad_p, uint32_t ad_d, const uint8_t *ro_p, uint32_t ro_d, const uint8_t *ao_p,
                               uint32_t ao_d, const uint8_t *gq_p, uint32_t gq_d) {
    UzVcfCell c = uz_vcf_cell_default();
    const uint32_t gt_t = gt_d & 15u, gt_n = gt_d >> 4, ad_t = ad_d & 15u, ad_n = ad_d >> 4, ro_t = ro_d & 15u, ro_n = ro_d >> 4, ao_t = ao_d & 15u,
                   ao_n = ao_d >> 4, gq_t = gq_d & 15u, gq_n = gq_d >> 4;
    if (gt_n) {
        if (!uz_bc_is_int(gt_t)) c.settled = false;
        else {
            int32_t al[2] = {-1, -1};
            int na = 0;
            for (uint32_t k = 0; k < gt_n && k < 2u; k++) { // (entries behind the second change nothing)
                int32_t x = 0;
                const int st = uz_bc_int(gt_t, gt_p, k, x);
                if (st == UZ_BC_EOV) break;
                al[na++] = st == UZ_BC_OK ? (x >> 1) - 1 : -1;
            }
            const int32_t a = al[0], b = al[1];
            if (na == 1) c.gt = a < 0 ? 2u : (a == 0 ? 0u : 3u);
            else if (na == 2) {
                if (a < 0 && b < 0) c.gt = 2u;
                else if (a < 0 || b < 0) c.gt = (b < 0 ? a : b) == 0 ? 0u : 1u;
                else if (a != b) c.gt = 1u;
                else c.gt = a == 0 ? 0u : 3u;
            }
        }
    }
    bool ad_done = false;
    if (ad_n) {
        if (!uz_bc_is_int(ad_t)) { c.settled = false; ad_done = true; }
        else {
            int32_t x0 = 0, x1 = 0;
            const int s0 = uz_bc_int(ad_t, ad_p, 0, x0);
            const int s1 = ad_n > 1u ? uz_bc_int(ad_t, ad_p, 1, x1) : UZ_BC_EOV;
            if (!(s0 != UZ_BC_OK && s1 == UZ_BC_EOV)) {
                c.settled &= uz_bc_depth(s0, x0, c.rd);
                c.settled &= uz_bc_depth(s1, x1, c.ad);
                ad_done = true;
            }
        }
    }
    if (!ad_done && ro_n && ao_n) {
        if (!uz_bc_is_int(ro_t) || !uz_bc_is_int(ao_t)) c.settled = false;
        else {
            int32_t x0 = 0, x1 = 0;
            const int s0 = uz_bc_int(ro_t, ro_p, 0, x0), s1 = uz_bc_int(ao_t, ao_p, 0, x1);
            c.settled &= uz_bc_depth(s0, x0, c.rd);
            c.settled &= uz_bc_depth(s1, x1, c.ad);
        }
    }
    if (gq_n) {
        if (gq_t == UZ_BC_FLOAT) {
            const uint32_t bits = uz_bc_load32(gq_p);
            if (bits != 0x7F800001u && bits != 0x7F800002u) {
                float f;
                memcpy(&f, &bits, 4);
                const float g = floorf(f);
                c.gq = !(g >= 0.0f) ? UZ_VC_MISSING : g > 32767.0f ? UZ_VC_MAX : (uint32_t)(int32_t)g;
            }
        } else if (uz_bc_is_int(gq_t)) {
            int32_t x = 0;
            if (uz_bc_int(gq_t, gq_p, 0, x) == UZ_BC_OK && x >= 0) c.gq = x > (int32_t)UZ_VC_MAX ? UZ_VC_MAX : (uint32_t)x;
        } else c.settled = false;
    }
    return c;
}

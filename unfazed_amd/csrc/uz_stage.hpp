// uz_stage.hpp -- what the sources that hold entry points share (abi.hip, tables.hip; not part of the ABI): the guard around an exported call, the
// staging of host columns into HBM (one copy per column, or one for a whole slab of them), the carving of a table's block, and the look-ups
// of the site, family and sample tables (tables.hip).
#pragma once
#include "uz_ctx.hpp"

// The message of a failed call.  uz_bgzf_inflate_to_host may run on a decoder's worker thread beside the owner's calls, so the
// context's message is written under a lock, and uz_last_error hands out a copy that belongs to the calling thread.
inline void set_error(uz_ctx *c, const std::string &msg) {
    std::lock_guard<std::mutex> lk(c->err_mu);
    c->err = msg;
}

template <typename F>
int guarded(uz_ctx *c, F &&fn) {
    if (!c) return UZ_E_ARG;
    try {
        (void)hipSetDevice(c->device);
        fn();
        return 0;
    } catch (const UzError &e) {
        set_error(c, e.msg);
        return e.code;
    } catch (const std::exception &e) {
        set_error(c, e.what());
        return UZ_E_ARG;
    } catch (...) {
        set_error(c, "unknown error");
        return UZ_E_ARG;
    }
}

// One copy instead of one per column: when the host columns of a table sit back to back in one slab of (pinned) memory --
// a decoder that carves its output from one allocation -- the slab goes over the link as a whole into a mirror block and
// the columns' device addresses follow from their offsets in it.  Every separate copy costs the link ~8 us of set-up, and
// a staged table has about twenty columns, half of them tiny.  A staging routine runs its h2d() calls twice: a planning
// pass that only looks at the host addresses, then -- mirrored or not -- the pass that yields the device pointers.
// the page-locked blocks this library handed out (uz_pinned_alloc, abi.hip): the one-copy path ships a span of host memory as a whole, so the
// span must lie inside ONE block the caller really owns -- never a guess from address density (columns of separate allocations
// that happen to sit close together, with unmapped or foreign memory between them)
bool inside_one_pinned_block(const uint8_t *lo, const uint8_t *hi);

struct SlabPlan {
    int mode = 1; // 1 planning, 2 mirrored
    const uint8_t *lo = nullptr, *hi = nullptr;
    size_t sum = 0;
    std::vector<const uint8_t *> at;
    uint8_t *dev = nullptr;
    void add(const void *p, size_t bytes) {
        const uint8_t *q = (const uint8_t *)p;
        if (!lo || q < lo) lo = q;
        if (!hi || q + bytes > hi) hi = q + bytes;
        sum += bytes;
        at.push_back(q);
    }
    size_t span() const { return (size_t)(hi - lo); }
    bool worth() const {
        if (at.size() < 2 || span() > sum + sum / 8 + 1024 * at.size()) return false;
        for (const uint8_t *q : at)
            if ((size_t)(q - lo) % 256) return false; // the kernels' vector loads want the carver's alignment
        return inside_one_pinned_block(lo, hi);
    }
};
inline thread_local SlabPlan *g_slab = nullptr;
struct SlabScope {
    explicit SlabScope(SlabPlan *p) { g_slab = p; }
    ~SlabScope() { g_slab = nullptr; }
};
inline const bool g_slab_off = getenv("UZ_NO_SLAB_COPY") != nullptr;

template <typename T>
const T *h2d(hipStream_t st, T *dst, const T *host, size_t n) {
    if (n) {
        UZ_REQUIRE(host != nullptr, UZ_E_ARG, "null column pointer");
        if (g_slab && g_slab->mode == 1) { g_slab->add(host, n * sizeof(T)); return dst; }
        if (g_slab && g_slab->mode == 2) return reinterpret_cast<const T *>(g_slab->dev + ((const uint8_t *)host - g_slab->lo));
        UZ_HIP(hipMemcpyAsync(dst, host, n * sizeof(T), hipMemcpyHostToDevice, st));
    }
    return dst;
}
// after the planning pass: ship the slab (mirror: the device block that receives it) or fall back to column copies
inline void slab_commit(uz_ctx *c, hipStream_t st, SlabPlan &plan, DevBlock &mirror) {
    if (!g_slab_off && plan.worth()) {
        mirror = uz_block_get(c, plan.span() + 512);
        UZ_HIP(hipMemcpyAsync(mirror.p, plan.lo, plan.span(), hipMemcpyHostToDevice, st));
        plan.dev = mirror.p;
        plan.mode = 2;
    } else
        g_slab = nullptr;
}

// carve arrays out of a table's block
struct Carver {
    uint8_t *base;
    size_t off = 0;
    explicit Carver(uint8_t *b) : base(b) {}
    template <typename T>
    T *take(size_t n) {
        off = (off + 255) & ~(size_t)255;
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += (n ? n : 1) * sizeof(T) + 64; // +64: vector tail reads stay in-bounds
        return p;
    }
};
// One pooled block, laid out by `layout` (no hipMalloc / hipFree per staged pass): it runs twice -- over a carver without memory, for the
// block's size, then over the block; the pointers it leaves behind are those of the second run
template <typename F>
DevBlock uz_carve(uz_ctx *c, F &&layout) {
    DevBlock blk;
    for (int pass = 0; pass < 2; pass++) {
        Carver cv(blk.p);
        layout(cv);
        if (!pass) blk = uz_block_get(c, cv.off + 256);
    }
    return blk;
}

// the tables behind the handles (tables.hip).  A look-up makes the compute stream wait for an asynchronous upload and runs the table's first-use
// work (the expansion of a link form, the complex flag folded into gt); a free releases everything a table owns: blocks, mirror and events
SitesDev &sites_of(uz_ctx *c, int id);
FamilyDev &fam_of(uz_ctx *c, int id);
SamplesDev &samples_of(uz_ctx *c, int id);
void free_sites(uz_ctx *c, SitesDev &s);
void free_family(uz_ctx *c, FamilyDev &f);
void free_samples(uz_ctx *c, SamplesDev &m);
// What needs the genotype columns of sites where the kid is not het -- the DEL / DUP classes, the columns themselves -- refuses a family
// that was staged in the het form
void refuse_het_only(const FamilyDev &f, const char *what);
// the window lists kept for family fam_id (-1: for every family) are forgotten (abi.hip)
void find_forget(uz_ctx *c, int fam_id);

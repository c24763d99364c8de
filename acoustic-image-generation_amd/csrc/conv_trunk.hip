// Host side of the pre-split (trunk) forward convolutions for gfx950 (MI355X): the ONE kernel selection (pick_trunk), the record
// of every trunk kernel with its LDS opt-in and cached occupancy (TrunkVariant), the tail planner, fwd_presplit behind the
// acimg_conv2d_fwd_split3p* / _split1p entries, the queries that report the selection, and the hooks of the ACIMG_STAMP /
// ACIMG_ABLATE diagnostic builds.  Shared with the other families: conv_host.hpp.
// Kernel headers (their rule: conv_host.hpp) this file owns, and alone includes: igemm_split3d_kernel.hpp (one tile per workgroup;
// its 128x128 / 128x64 instances are compiled in conv_tiles.hip: conv_tiles.hpp says why), igemm_split3dp_kernel.hpp (persistent;
// the two-pass epilogues), igemm_split3r_kernel.hpp (ring), igemm_split3h_kernel.hpp (halo).
#include "conv_host.hpp"
#include "conv_tiles.hpp"
#include "igemm_split3dp_kernel.hpp"
#include "igemm_split3r_kernel.hpp"
#include "igemm_split3h_kernel.hpp"
#include <algorithm>

namespace acimg {

// ---- which kernel a pre-split (trunk) forward conv runs on: the ONE place that decides it.  fwd_presplit launches what
// pick_trunk says; acimg_conv2d_fwd_split3p_stats_rows and acimg_conv2d_fwd_split3_tiling report it ----
enum TrunkKind { TRUNK_ONE_TILE = 0, TRUNK_PERSISTENT = 1, TRUNK_RING = 2, TRUNK_HALO = 3 };   // = the tiling query's third word
struct TrunkPick {
    TrunkKind kind;
    int bm, bn;          // row and column tile
    int stats_rows;      // statistics partials the kernel leaves: one per row tile
    bool big_out;        // the output exceeds a 32-bit buffer descriptor
};

// Halo kernel (igemm_split3h_kernel.hpp) for a pre-split trunk conv: 3x3 / stride 1 / SAME on 128x128 tiles, image rows
// short enough for an 18-brick patch.  trunk_halo = 1 takes it where it was measured to pay, 2 wherever it applies.
static constexpr int HALO_NB = 18;
static bool halo_applies(const AcimgConvDesc* d, int terms, const Split3Cfg& c) {
    if (terms != 3 || d->R != 3 || d->S != 3 || d->stride != 1 || d->pad_t != 1 || d->pad_l != 1 || d->OH != d->H ||
        d->OW != d->W || d->C % 32)
        return false;
    if (c.bm != 128 || c.bn != 128) return false;
    return ((d->W + 16) >> 4) + 8 + (d->W >> 4) + 1 <= HALO_NB;
}

static TrunkPick pick_trunk(const AcimgConvDesc* d, int terms, bool two_pass) {
    const int M = d->N * d->OH * d->OW;
    const Split3Cfg c = pick_split3(M, d->K);
    const bool t128 = c.bm == 128 && c.bn == 128;
    // the persistent and the ring kernel address the output through a 32-bit buffer descriptor; a larger output (per-GPU
    // batches around 512 on the first trunk units) falls back to the one-tile kernel's 64-bit pointer stores
    TrunkPick t{TRUNK_ONE_TILE, c.bm, c.bn, 0, (long)M * d->ldy * 4 >= (1L << 31)};
    // statistics-only / fused-tail passes: always the persistent kernel (whole tiles, then K ranges of the tail tiles);
    // fwd_presplit refuses the shapes that kernel does not take
    if (two_pass) t.kind = TRUNK_PERSISTENT;
    // trunk_halo = 1 ("where it was measured to pay") selects nothing yet: at batch 32 the halo form is at parity with the
    // per-tap kernels on the 56x75 / 28x38 layers and behind the ring kernel on 14x19; 2 = wherever it applies
    else if (g_cfg.trunk_halo == 2 && halo_applies(d, terms, c)) t.kind = TRUNK_HALO;
    // Ring kernel (igemm_split3r_kernel.hpp) for a pre-split trunk conv, and with how many tile rows (ring_rows; 0 = not on it).
    // Measured per shape at batch 32 and 30 (tools/trunk_shapes.py, profiles/r03/trunk_shapes_r03*.txt): in its steady state
    // the ring kernel's K loop is 8-14 % faster than the two-workgroups-per-CU kernels' (long-K layers whose tiles fill one
    // round of the 256 CUs), but with ONE workgroup per CU it pays more for tile quantisation (a 1.04-round layer leaves
    // 246 CUs idle for a round, where 512 slots leave a quarter of the chip) and for short-K tiles (the output tile's stores
    // and the deferred stage at every unit boundary).  trunk_ring = 1 therefore takes it where it won: layers of at most
    // ~1.2 rounds of 128x128 tiles over the CUs (the 14x19 stage) with at least 64 K steps, on 128-row tiles with the tail
    // cut into K ranges; trunk_ring = 2 forces it (experiments, tests).
    int ring_rows = 0;
    if (!two_pass && t.kind != TRUNK_HALO && !t.big_out && g_cfg.trunk_ring && terms == 3 && t128) {
        const long t128s = (long)cdiv(M, 128) * cdiv(d->K, 128);
        const int kiters = d->R * d->S * (d->C / 32);
        const long t256 = (long)cdiv(M, 256) * cdiv(d->K, 128);
        if (g_cfg.trunk_ring == 1) ring_rows = (t128s > 256 && t128s <= 300 && kiters >= 64) ? 128 : 0;
        else if (g_cfg.trunk_ring_bm) ring_rows = g_cfg.trunk_ring_bm;
        else ring_rows = t256 >= 500 ? 256 : 128;
    }
    if (ring_rows) {
        t.kind = TRUNK_RING;
        t.bm = ring_rows;
    }
    // Persistent kernel or one tile per workgroup for the pre-split (trunk) forward conv (tools/trunk_shapes.py,
    // profiles/r02/trunk_shapes_*.txt): walking a tile list wins 2-9 % wherever there is at least one full round of whole
    // 128x128 tiles (most on short-K multi-round layers); when every tile belongs to the split tail (fewer tiles than
    // resident workgroups) the one-tile kernel's leaner code is 3-7 % faster.
    const long tiles = (long)cdiv(M, c.bm) * cdiv(d->K, c.bn);
    if (t.kind == TRUNK_ONE_TILE && !t.big_out && t128 && (g_cfg.trunk_persistent == 2 || (g_cfg.trunk_persistent == 1 && tiles >= 512)))
        t.kind = TRUNK_PERSISTENT;
    t.stats_rows = cdiv(M, t.bm);
    return t;
}

// ---- tail split of the trunk kernel: which tiles to cut, and into how many K ranges ------------------------
struct TailPlan { int whole, s, rem; };

// One record per trunk kernel that is launched: what a launch and the occupancy question need to know about it, and what
// was learnt about it in this process (both once per process).
struct TrunkVariant {
    const void* fn;
    int threads;
    size_t lds;                  // dynamic LDS bytes of a launch
    int wgs_per_cu;              // resident workgroups per CU assumed when no device answers
    bool lds_opt_in;             // its dynamic LDS exceeds 64 KiB: needs the opt-in once per process
    TrunkVariant* slots_of;      // the sibling whose occupancy stands for this kernel's (nullptr: its own)
    int slots;                   // resident workgroups on the device, 0 = not asked yet
    bool opted_in;
};
// one-tile kernels: 2 stages x (hi, lo) x 64-byte rows; the epilogue restages the fp32 output tile there (+ 2 x WGM x BN
// floats of statistics scratch behind it)
static constexpr size_t tile_lds(size_t bm, size_t bn) { return std::max(2 * 2 * (bm + bn) * 64, bm * bn * 4) + 4 * 2 * bn * 4; }
// (a 64-deep K step - whole 128-byte operand rows, one workgroup per CU - was measured slower on every trunk shape in
//  round 2 and removed when the operands moved to LDS-tile order, which gives whole-line requests at two per CU)
static constexpr size_t PERSISTENT_LDS = (size_t)2 * 4 * 128 * 64 + 4 * 2 * 128 * 4;    // 2 stages + statistics scratch
static constexpr size_t ring_lds(size_t rows) { return 3 * 2 * (rows + 128) * 64 + 4 * 2 * 128 * 4; }
static constexpr size_t HALO_LDS = (size_t)2 * (HALO_NB * 1024 + 64) + 2 * 2 * 128 * 64;
#define ACIMG_KFN(...) reinterpret_cast<const void*>(__VA_ARGS__)
static TrunkVariant TILE_128x128 = {ACIMG_KFN(igemm_split3d_kernel<128, 128, 2, 4, 512, 2, 2>), 512, tile_lds(128, 128), 2, false, nullptr};
static TrunkVariant TILE_64x128 = {ACIMG_KFN(igemm_split3d_kernel<64, 128, 1, 4, 256, 2, 2>), 256, tile_lds(64, 128), 3, false, nullptr};
static TrunkVariant TILE_128x64 = {ACIMG_KFN(igemm_split3d_kernel<128, 64, 2, 2, 256, 2, 2>), 256, tile_lds(128, 64), 3, false, nullptr};
static TrunkVariant TILE1_128x128 = {ACIMG_KFN(igemm_split3d_kernel<128, 128, 2, 4, 512, 2, 2, 1>), 512, tile_lds(128, 128), 2, false, &TILE_128x128};
static TrunkVariant TILE1_64x128 = {ACIMG_KFN(igemm_split3d_kernel<64, 128, 1, 4, 256, 2, 2, 1>), 256, tile_lds(64, 128), 3, false, &TILE_64x128};
static TrunkVariant TILE1_128x64 = {ACIMG_KFN(igemm_split3d_kernel<128, 64, 2, 2, 256, 2, 2, 1>), 256, tile_lds(128, 64), 3, false, &TILE_128x64};
static TrunkVariant PERSISTENT = {ACIMG_KFN(igemm_split3dp_kernel<32, 0>), 512, PERSISTENT_LDS, 2, false, nullptr};
static TrunkVariant PERSISTENT_SPREAD = {ACIMG_KFN(igemm_split3dp_kernel<32, 1>), 512, PERSISTENT_LDS, 2, false, &PERSISTENT};
static TrunkVariant PERSISTENT1 = {ACIMG_KFN(igemm_split3dp_kernel<32, 0, 1>), 512, PERSISTENT_LDS, 2, false, &PERSISTENT};
static TrunkVariant PASS_STATS = {ACIMG_KFN(igemm_split3dp_kernel<32, 0, 3, 1>), 512, PERSISTENT_LDS, 2, false, nullptr};
static TrunkVariant PASS_TAIL = {ACIMG_KFN(igemm_split3dp_kernel<32, 0, 3, 2>), 512, PERSISTENT_LDS, 2, false, nullptr};
static TrunkVariant PASS_TAIL_PROJ = {ACIMG_KFN(igemm_split3dp_kernel<32, 0, 3, 3>), 512, PERSISTENT_LDS, 2, false, nullptr};
static TrunkVariant RING_256 = {ACIMG_KFN(igemm_split3r_kernel<4>), 512, ring_lds(256), 1, true, nullptr};
static TrunkVariant RING_128 = {ACIMG_KFN(igemm_split3r_kernel<2>), 512, ring_lds(128), 1, true, nullptr};
static TrunkVariant HALO = {ACIMG_KFN(igemm_split3h_kernel<HALO_NB>), 512, HALO_LDS, 2, true, nullptr};
#undef ACIMG_KFN

static void opt_in_lds(TrunkVariant& v) {
    if (!v.lds_opt_in || v.opted_in) return;
    (void)hipFuncSetAttribute(v.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds);
    v.opted_in = true;
}
// workgroups of `v` the device holds at once (the occupancy question is only answered for a kernel that may use its LDS:
// it is opted in first)
static int resident_slots(TrunkVariant& v) {
    opt_in_lds(v);
    TrunkVariant& o = v.slots_of ? *v.slots_of : v;
    if (!o.slots) {
        int dev = 0, ncu = 0, per = 0;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, o.fn, o.threads, v.lds) != hipSuccess || ncu <= 0 || per <= 0) {
            (void)hipGetLastError();
            ncu = 256;                    // MI355X; no device (CPU-side sizing queries): same answer
            per = o.wgs_per_cu;
        }
        o.slots = ncu * per;
    }
    return o.slots;
}
// `units` and `cap` reach the kernels that walk a unit list (persistent, ring).  The one-tile and halo kernels take p alone:
// the runtime reads as many argument pointers as the kernel's metadata declares, so the two spare ones are never touched.
// The launch's status is left to the caller's check_launch (hipGetLastError), as after hipLaunchKernelGGL.
static void launch_trunk(const TrunkVariant& v, int nwg, hipStream_t st, IgemmParams& p, int units = 0, int cap = 0) {
    void* args[] = {&p, &units, &cap};
    (void)hipLaunchKernel(v.fn, dim3(nwg), dim3(v.threads), args, v.lds, st);
}
static TailPlan pick_tail(int T, int P, int KI, int max_units) {
    const int rem = T % P;
    TailPlan best{T, 1, 0};
    if (rem == 0 || !g_cfg.tail_split) return best;
    if (g_cfg.tail_s) {   // experiments only: force the number of K ranges
        const int s = g_cfg.tail_s;
        if (s > 1 && KI / s >= 1 && (long)rem * s <= max_units) return TailPlan{T - rem, s, rem};
        return best;
    }
    // cost in K steps of the last round: whole tiles = KI; s ranges = rounds(rem*s) * ceil(KI/s) + hand-off
    double best_cost = KI;
    static const int cand[] = {2, 3, 4, 6, 8, 12, 16};
    for (int s : cand) {
        if (KI / s < 2 || (long)rem * s > max_units) break;
        // hand-off calibrated on the trunk shapes (tools/tune_dma.py): partial store + ticket + the last arriver's
        // s x 64 KiB of sc1 loads cost about 8 + s K steps, so 1x1 layers with few K steps are left whole
        const double cost = (double)cdiv((long)rem * s, P) * cdiv(KI, s) + 8.0 + 1.0 * s;
        if (cost < 0.9 * best_cost) {
            best_cost = cost;
            best = TailPlan{T - rem, s, rem};
        }
    }
    return best;
}
static constexpr int TS_MAX_UNITS = 1024;      // partial slots (64 KiB each for a 128x128 tile; a 256x128 tile takes two)
static constexpr size_t TS_COUNTER_BYTES = 4096;
static constexpr size_t TS_WS_BYTES = TS_COUNTER_BYTES + (size_t)TS_MAX_UNITS * 128 * 128 * sizeof(float);   // acimg_conv2d_fwd_split3p_workspace

// Tail wiring of a trunk launch: with the caller's workspace (and a kernel that takes the split: `allow`) the tiles of the
// last, partial round over `slots` workgroups are cut into K ranges; the ticket counters and partial slots are wired either
// way.  Returns the number of work units: whole tiles + K ranges.
static int wire_tail(IgemmParams& p, void* ws, size_t ws_bytes, int tiles, int slots, int max_units, bool allow) {
    TailPlan t{tiles, 1, 0};
    if (allow && ws && ws_bytes >= TS_WS_BYTES) t = pick_tail(tiles, slots, p.kiters, max_units);
    p.ts_whole = t.whole; p.ts_s = t.s;
    p.ts_counters = static_cast<int*>(ws);
    p.ts_partial = ws ? reinterpret_cast<float*>(static_cast<char*>(ws) + TS_COUNTER_BYTES) : nullptr;
    return t.whole + t.rem * t.s;
}

#if defined(ACIMG_STAMP) || defined(ACIMG_ABLATE)
static float* g_stamp_buf = nullptr;      // diagnostic build only (tools/build_stamp.sh): never in libacimg.so
static int g_stamp_nostore = 0;           // ablation: the persistent kernel's output stores go out of range (dropped)
#endif

// the two passes of a conv whose raw output never reaches memory (igemm_split3dp_kernel, EPI 1 / 2)
struct Split3pTail {
    int mode;                      // 1: statistics only; 2: relu(acc * scale + shift + shortcut) -> split planes;
                                   // 3: the same with a projection shortcut (raw fp32 + its own scale / shift)
    const float* scale;
    const float* shift;
    const void* sc_planes;         // mode 3: the fp32 [M][K] output of the shortcut conv
    size_t sc_lo_off;
    void* out_planes;
    size_t out_lo_off;
    const float* scale2;
    const float* shift2;
};

static int fwd_presplit(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit, float* y,
                        float* stats, void* ws, size_t ws_bytes, void* stream, const int terms,
                        const Split3pTail* tail = nullptr) {
    int rc = check_desc(d, "conv2d_fwd_split3p");
    if (rc) return rc;
    if (d->C % 32) return fail(ACIMG_EINVAL, "conv2d_fwd_split3p: C=%d must be a multiple of 32", d->C);
    // (y here is a wide-access operand: the trunk kernels store whole 16-byte pieces, include/acimg.h)
    if ((rc = check_wide("conv2d_fwd_split3p", {{"x_planes", x_planes}, {"wsplit", wsplit}, {"y", y}})) ||
        (rc = check_wide_ld("conv2d_fwd_split3p", {{"ldy", d->ldy}})) || (rc = check_ws_aligned("conv2d_fwd_split3p", ws)))
        return rc;
    if (d->ldw < d->K || d->ldx != d->C || (x_lo_off & 15))
        return fail(ACIMG_EINVAL, "conv2d_fwd_split3p: ldw<K, ldx != C (split-format tensors are dense) or x_lo_off not a multiple of 16");
    IgemmParams p = fwd_view(d);
    split_ksteps(p);
    p.A = static_cast<const float*>(x_planes); p.B = static_cast<const float*>(wsplit);
    const long plane = (long)acimg_split_plane_bytes((long)d->N * d->H * d->W, d->C);
    const long a_bytes = (long)x_lo_off + plane;
    const long b_bytes = (long)acimg_conv2d_split3_weight_bytes(d);
    if (a_bytes >= (1L << 31) || b_bytes >= (1L << 31) || (long)x_lo_off < plane)
        return fail(ACIMG_EINVAL, "conv2d_fwd_split3p: operand >= 2 GiB or overlapping planes");
    p.a_bytes = (unsigned)a_bytes; p.b_bytes = (unsigned)b_bytes; p.a_lo_off = (unsigned)x_lo_off;
    p.b_brick = (unsigned)split3_rowmajor_bytes(d);
    EpiParams& e = p.e;
    e.Y = y; e.stats = stats; e.vec = 1;
    const TrunkPick t = pick_trunk(d, terms, tail != nullptr);
    hipStream_t st = (hipStream_t)stream;
    // XCD-aware rasterisation: the ~64 tiles resident on one XCD (32 of the ring kernel's, one workgroup per CU) form a
    // (64/gn) x gn rectangle of the tile grid
    p.ras_tiles_m = cdiv(p.M, t.bm);
    p.ras_tiles_n = cdiv(d->K, t.bn);
    p.ras_gn = std::min(p.ras_tiles_n, 8);
    p.ras_gm = std::max(1, (t.kind == TRUNK_RING ? 32 : 64) / p.ras_gn);
    const int T = p.ras_tiles_m * p.ras_tiles_n;
    const bool t128 = t.bm == 128 && t.bn == 128;
    if (tail) {
        if (terms != 3 || !t128 || t.big_out || d->K % 128 || d->ldy != d->K || d->ldw != d->K)
            return fail(ACIMG_EINVAL, "conv2d_fwd_split3p (two-pass): needs 128x128 tiles, K %% 128 == 0, dense output < 2 GiB");
        TrunkVariant& v = tail->mode == 1 ? PASS_STATS : tail->mode == 2 ? PASS_TAIL : PASS_TAIL_PROJ;
        const int slots = resident_slots(v);
        const int units = wire_tail(p, ws, ws_bytes, T, slots, TS_MAX_UNITS, true);
        const int nwg = std::min(units, slots);
        const char* what = "conv2d_fwd_split3p_stats";
        e.Y = nullptr;
        if (tail->mode != 1) {
            const long oplane = (long)acimg_split_plane_bytes((long)p.M, d->K);
            if ((rc = check_wide("conv2d_fwd_split3p_tail", {{"shortcut", tail->sc_planes}, {"out_planes", tail->out_planes}}))) return rc;
            if ((tail->out_lo_off & 15) ||
                (long)tail->out_lo_off < oplane || (long)tail->out_lo_off + oplane >= (1L << 31))
                return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_tail: unaligned / overlapping / >= 2 GiB split-format operands");
            e.stats = nullptr;
            e.f_scale = tail->scale; e.f_shift = tail->shift;
            e.f_sc = static_cast<const char*>(tail->sc_planes);
            e.f_out = static_cast<char*>(tail->out_planes); e.f_out_lo = (unsigned)tail->out_lo_off;
            e.f_out_bytes = (unsigned)(tail->out_lo_off + oplane);
            if (tail->mode == 3) {
                e.f_scale2 = tail->scale2; e.f_shift2 = tail->shift2;
                e.f_sc_lo = 0; e.f_sc_bytes = (unsigned)((long)p.M * d->K * 4);      // < 2 GiB: big_out was refused above
                what = "conv2d_fwd_split3p_tail_proj";
            } else {
                if ((tail->sc_lo_off & 15) || (long)tail->sc_lo_off < oplane || (long)tail->sc_lo_off + oplane >= (1L << 31))
                    return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_tail: unaligned / overlapping / >= 2 GiB shortcut planes");
                e.f_sc_lo = (unsigned)tail->sc_lo_off;
                e.f_sc_bytes = (unsigned)(tail->sc_lo_off + oplane);
                what = "conv2d_fwd_split3p_tail";
            }
        }
        launch_trunk(v, nwg, st, p, units, nwg);
        return check_launch(what);
    }
    if (t.kind == TRUNK_HALO) {
        // one tile per workgroup, K walked as (channel chunk, tap) over one staged patch per chunk; tail tiles in K ranges
        const int units = wire_tail(p, ws, ws_bytes, T, resident_slots(HALO), TS_MAX_UNITS, true);
        launch_trunk(HALO, units, st, p);
        return check_launch("conv2d_fwd_split3p (halo)");
    }
#if defined(ACIMG_STAMP) || defined(ACIMG_ABLATE)
    p.slab = g_stamp_buf;
    p.flip = g_stamp_nostore;
#endif
    if (t.kind == TRUNK_RING) {
        // one workgroup per CU walks units blockIdx.x, blockIdx.x + P, ... (whole tiles, then K ranges of the tail tiles)
        TrunkVariant& v = t.bm == 256 ? RING_256 : RING_128;
        const int slots = resident_slots(v);
        const int units = wire_tail(p, ws, ws_bytes, T, slots, TS_MAX_UNITS * 128 / t.bm, true);
        const int nwg = std::min(units, slots);
        p.splits = g_cfg.trunk_stagger > 0 ? 2 : 1;   // ring kernel: waves 4-7 do a step's scalar work before their first MFMA group
        launch_trunk(v, nwg, st, p, units, nwg);
        return check_launch("conv2d_fwd_split3p (ring)");
    }
    if (t.kind == TRUNK_PERSISTENT) {
        TrunkVariant& v = terms == 1 ? PERSISTENT1 : g_cfg.trunk_dma_pos == 1 ? PERSISTENT_SPREAD : PERSISTENT;
        const int slots = resident_slots(v);
        const int units = wire_tail(p, ws, ws_bytes, T, slots, TS_MAX_UNITS, true);
        p.splits = g_cfg.trunk_stagger > 0 ? g_cfg.trunk_stagger * (p.kiters * 2500 + 8000) / 100 : 1;
        // a workgroup per resident slot walks units blockIdx.x, blockIdx.x + P, ...: whole tiles first (with the
        // next tile's first operand stage and addresses prepared under the current tile's last K step and output
        // stores), then the K ranges of the tail tiles
        const int nwg = std::min(units, slots);
        launch_trunk(v, nwg, st, p, units, nwg);
        return check_launch("conv2d_fwd_split3p");
    }
    // one tile (or K range of a tail tile) per workgroup
    TrunkVariant& v = t128 ? (terms == 1 ? TILE1_128x128 : TILE_128x128)
                    : t.bm == 64 ? (terms == 1 ? TILE1_64x128 : TILE_64x128) : (terms == 1 ? TILE1_128x64 : TILE_128x64);
    const int units = wire_tail(p, ws, ws_bytes, T, resident_slots(v), TS_MAX_UNITS, t128);
    launch_trunk(v, units, st, p);
    return check_launch("conv2d_fwd_split3p");
}

}  // namespace acimg

using namespace acimg;

extern "C" {      // ---- C ABI ----

int acimg_conv2d_fwd_split3p_stats_rows(const AcimgConvDesc* d) { return pick_trunk(d, 3, false).stats_rows; }

int acimg_conv2d_fwd_split3_tiling(const AcimgConvDesc* d, int* out) {
    if (!d || !out) return fail(ACIMG_EINVAL, "conv2d_fwd_split3_tiling: null argument");
    const TrunkPick t = pick_trunk(d, 3, false);
    out[0] = t.bm;
    out[1] = t.bn;
    out[2] = t.kind;
    return ACIMG_OK;
}

size_t acimg_conv2d_fwd_split3p_workspace(const AcimgConvDesc* d) {
    (void)d;
    return TS_WS_BYTES;
}

#if defined(ACIMG_STAMP) || defined(ACIMG_ABLATE)
int acimg_debug_stamp_buffer(void* buf) {
    g_stamp_buf = static_cast<float*>(buf);
    return 0;
}
int acimg_debug_no_output_stores(int on) {
    g_stamp_nostore = on;
    return 0;
}
#endif

int acimg_conv2d_fwd_split3p(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                             float* y, float* stats, void* ws, size_t ws_bytes, void* stream) {
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, y, stats, ws, ws_bytes, stream, 3);
}

int acimg_conv2d_fwd_split1p(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                             float* y, float* stats, void* ws, size_t ws_bytes, void* stream) {
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, y, stats, ws, ws_bytes, stream, 1);
}

int acimg_conv2d_fwd_split3p_stats(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                                   float* stats, void* ws, size_t ws_bytes, void* stream) {
    if (!stats) return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_stats: null statistics buffer");
    const Split3pTail t{1, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr};
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, nullptr, stats, ws, ws_bytes, stream, 3, &t);
}

int acimg_conv2d_fwd_split3p_tail(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                                  const float* scale, const float* shift, const void* sc_planes, size_t sc_lo_off,
                                  void* out_planes, size_t out_lo_off, void* ws, size_t ws_bytes, void* stream) {
    if (!scale || !shift || !sc_planes || !out_planes)
        return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_tail: null scale, shift, shortcut or output");
    if (int rc = check_wide("conv2d_fwd_split3p_tail", {{"scale", scale}, {"shift", shift}})) return rc;
    const Split3pTail t{2, scale, shift, sc_planes, sc_lo_off, out_planes, out_lo_off, nullptr, nullptr};
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, nullptr, nullptr, ws, ws_bytes, stream, 3, &t);
}

int acimg_conv2d_fwd_split3p_tail_proj(const AcimgConvDesc* d, const void* x_planes, size_t x_lo_off, const void* wsplit,
                                       const float* scale, const float* shift, const float* sc32, const float* sc_scale,
                                       const float* sc_shift, void* out_planes, size_t out_lo_off, void* ws, size_t ws_bytes,
                                       void* stream) {
    if (!scale || !shift || !sc32 || !sc_scale || !sc_shift || !out_planes)
        return fail(ACIMG_EINVAL, "conv2d_fwd_split3p_tail_proj: null scale, shift, shortcut or output");
    if (int rc = check_wide("conv2d_fwd_split3p_tail_proj", {{"scale", scale}, {"shift", shift}, {"sc_scale", sc_scale}, {"sc_shift", sc_shift}}))
        return rc;
    const Split3pTail t{3, scale, shift, sc32, 0, out_planes, out_lo_off, sc_scale, sc_shift};
    return fwd_presplit(d, x_planes, x_lo_off, wsplit, nullptr, nullptr, ws, ws_bytes, stream, 3, &t);
}

}  // extern "C"

// kernels_fuse.hip -- voxel-grid fusion of organised point clouds (slr_fuse_voxels): every point of every (aligned) frame falls
// into a cubic cell, every occupied cell with enough members becomes one point -- the centroid of its members -- with a member
// count (and a mean grey value).  The step the reference prepares and never takes: MFReconstruct::triangulation moves every scan
// into the first one's frame "for stitching" (mfreconstruct.cpp:276-323), MainWindow::startreconstruct then writes one PLY per
// scan (mainwindow.cpp:632-645).  gfx950 (MI355X) only.
//
// Exact integer accumulation, so the result is bit-reproducible whatever the order of the atomics: a point's in-cell position is
// quantised to 24 bits per axis and summed in u64; the centroid is formed once at the end in f64 (include/slr.h gives the formulas).
// Passes (one launch each, on the ctx stream):
//   clear    the open-addressing table (power of two >= 2 max_voxels entries of 48 B) to the all-ones key, and the counter shards;
//   insert   one thread per point; the 64 consecutive points of a wave are grouped by equal voxel keys (a ballot per distinct
//            key, a wave sum per group of more than one), and only a group's leader probes the table (64-bit CAS on the key) and
//            adds the group's count / sums / colour (cdna_hip_programming.md Guideline 12); new keys are counted per wave into
//            256 shards;
//   total    one workgroup sums the shards: distinct voxels, rejected points, atomics (debug);
//   flag     one thread per point, the same groups: a group's leader looks its key up (read-only probe) and flags itself when it is the
//            cell's first member and the cell has min_points members -- a u8 flag image in point order;
//   scan     the flag image through kernels_compact.hip's scan (flag_count / block_scan / flag_index): the flagged points'
//            positions, in point order = ascending `first`, with no sort;
//   emit     one thread per output voxel: re-derives its key from the first member, looks the cell up, writes centroid, count, colour.
// Every probe loop is bounded (by min(table size, max_voxels + 1): a longer chain proves more than max_voxels distinct keys), and
// the insert gives up once the published distinct count exceeds max_voxels (flag: abort); the flag pass flags nothing when the
// total exceeds max_voxels, so the emit pass never writes past the caller's capacity.
#include "slr_device.hpp"

namespace slr {

constexpr int kFuseBlock = 256;
constexpr unsigned kFuseShards = 256;
constexpr unsigned long long kFuseEmpty = ~0ull;     // all-ones key: no voxel packs to it (bit 63 is always 0)
constexpr double kFuseQ = 16777216.0;                // 2^24: in-cell quantisation
constexpr double kFuseRange = 1048576.0;             // 2^20: cell indices in [-2^20, 2^20) per axis (21 bits)

struct FuseEntry { unsigned long long key, S[3], csum; unsigned count, first; };                 // 48 B
struct FuseShard { unsigned long long rejected, atomics; unsigned claims, pad[27]; };            // 128 B: one line each
static_assert(sizeof(FuseEntry) == 48 && sizeof(FuseShard) == 128, "layout");
static_assert(kFuseShards == (unsigned)kFuseBlock, "the clear kernel's first workgroup zeroes one shard per thread");

size_t fuse_table_entries(uint32_t max_voxels)
{
    size_t t = 1024;
    while (t < 2 * (size_t)max_voxels) t <<= 1;
    return t;
}
size_t fuse_table_bytes(uint32_t max_voxels) { return fuse_table_entries(max_voxels) * sizeof(FuseEntry); }
size_t fuse_stats_bytes() { return kFuseShards * sizeof(FuseShard) + sizeof(FuseTotals); }

struct FuseArgs {
    const float *xyz; const uint8_t *has; const uint8_t *color; const float *T;
    size_t n; unsigned frame_px;
    double voxel, org[3];
    FuseEntry *table; unsigned long long mask; unsigned bound;
    unsigned max_voxels, min_points;
    FuseShard *shards; FuseTotals *tot; int count_atomics;
};

__device__ __forceinline__ unsigned long long fuse_hash(unsigned long long k)      // splitmix64's finaliser
{
    k ^= k >> 31; k *= 0x7fb5d329728ea185ull;
    k ^= k >> 27; k *= 0x81dadef4bc2dd44dull;
    k ^= k >> 33;
    return k;
}

// point e -> packed voxel key ((v_a + 2^20) in bits 21 a .. 21 a + 20) and in-cell positions q_a in [0, 2^24);
// false: the point is rejected (a non-finite coordinate, or a cell index outside [-2^20, 2^20))
__device__ __forceinline__ bool fuse_key(const FuseArgs &a, unsigned e, unsigned long long *key, unsigned q[3])
{
    float X[3] = {a.xyz[3 * (size_t)e], a.xyz[3 * (size_t)e + 1], a.xyz[3 * (size_t)e + 2]};
    if (a.T) apply_T(a.T + 12 * (size_t)(e / a.frame_px), X);
    if (!__builtin_isfinite(X[0]) || !__builtin_isfinite(X[1]) || !__builtin_isfinite(X[2])) return false;
    unsigned long long k = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
        const double g = ((double)X[ax] - a.org[ax]) / a.voxel;
        const double v = __builtin_floor(g);
        if (!(v >= -kFuseRange && v < kFuseRange)) return false;
        q[ax] = (unsigned)((g - v) * kFuseQ);
        k |= (unsigned long long)((long long)v + (1ll << 20)) << (21 * ax);
    }
    *key = k;
    return true;
}

// the wave's groups of equal keys (any lanes, not only neighbours: the depth of a reconstructed row jitters between two cells):
// the leader of a group is its lowest lane = its smallest point index.  Lanes with ok == false belong to no group.
// f(lane_is_member, leader_lane, member_mask) is called once per group, wave-uniformly.
template <typename F>
__device__ __forceinline__ void fuse_groups(bool ok, unsigned long long key, F f)
{
    unsigned long long pending = __ballot(ok);
    while (pending) {
        const int l = __ffsll((long long)pending) - 1;
        const unsigned long long lk = __shfl(key, l);
        const bool mine = ok && key == lk;
        const unsigned long long m = __ballot(mine);
        f(mine, l, m);
        pending &= ~m;
    }
}

// read-only probe; null: the key is not in the table within `bound` probes
__device__ __forceinline__ const FuseEntry *fuse_find(const FuseArgs &a, unsigned long long key)
{
    unsigned long long h = fuse_hash(key) & a.mask;
    for (unsigned s = 0; s < a.bound; s++, h = (h + 1) & a.mask) {
        const unsigned long long cur = __hip_atomic_load(&a.table[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == key) return a.table + h;
        if (cur == kFuseEmpty) return nullptr;
    }
    return nullptr;
}

__global__ __launch_bounds__(kFuseBlock) void fuse_clear_kernel(FuseEntry *__restrict__ table, size_t entries,
                                                                FuseShard *__restrict__ shards, FuseTotals *__restrict__ tot)
{
    const size_t i = (size_t)blockIdx.x * kFuseBlock + threadIdx.x;
    if (i < entries) {
        FuseEntry z;
        z.key = kFuseEmpty; z.S[0] = z.S[1] = z.S[2] = 0; z.csum = 0; z.count = 0; z.first = 0xFFFFFFFFu;
        table[i] = z;
    }
    if (blockIdx.x == 0) {
        shards[threadIdx.x].rejected = 0; shards[threadIdx.x].atomics = 0; shards[threadIdx.x].claims = 0;
        if (threadIdx.x == 0) { tot->rejected = 0; tot->atomics = 0; tot->ndist = 0; tot->abort = 0; tot->emitted = 0; }
    }
}

// the published distinct count exceeds max_voxels (claims still in flight are missing from it: it never overstates)
__device__ __noinline__ bool fuse_overflowed(const FuseShard *shards, unsigned max_voxels)
{
    unsigned long long s = 0;
    for (unsigned k = 0; k < kFuseShards; k++) s += __hip_atomic_load(&shards[k].claims, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return s > max_voxels;
}

__global__ __launch_bounds__(kFuseBlock) void fuse_insert_kernel(FuseArgs a)
{
    const int lane = threadIdx.x & 63;
    if (__hip_atomic_load(&a.tot->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;     // wave-uniform
    const size_t e64 = (size_t)blockIdx.x * kFuseBlock + threadIdx.x;
    const unsigned e = (unsigned)e64;
    FuseShard *sh = a.shards + ((blockIdx.x * (kFuseBlock / 64) + (threadIdx.x >> 6)) & (kFuseShards - 1));
    unsigned long long key = kFuseEmpty;
    unsigned q[3] = {0, 0, 0}, col = 0;
    bool ok = false, rej = false;
    if (e64 < a.n && a.has[e]) {
        ok = fuse_key(a, e, &key, q);
        rej = !ok;
        if (ok && a.color) col = a.color[e];
    }
    const unsigned long long rejm = __ballot(rej);
    if (lane == 0 && rejm) atomicAdd(&sh->rejected, (unsigned long long)__popcll(rejm));
    if (!ok) key = kFuseEmpty;
    if (!__ballot(ok)) return;                                                                     // wave-uniform
    // one total per group, held by its leader (sums over at most 64 members: q <= 64 (2^24 - 1) < 2^32)
    bool lead = false;
    unsigned s0 = 0, s1 = 0, s2 = 0, cc = 0;         // count (<= 64) in bits 0..7, colour sum (<= 16320) above
    fuse_groups(ok, key, [&](bool mine, int l, unsigned long long m) {
        unsigned v0 = mine ? q[0] : 0u, v1 = mine ? q[1] : 0u, v2 = mine ? q[2] : 0u, v3 = mine ? 1u + (col << 8) : 0u;
        if (m & (m - 1)) {                           // more than one member: a wave sum (singletons keep their own values)
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) {
                v0 += __shfl_xor(v0, d); v1 += __shfl_xor(v1, d); v2 += __shfl_xor(v2, d); v3 += __shfl_xor(v3, d);
            }
        }
        if (lane == l) { lead = true; s0 = v0; s1 = v1; s2 = v2; cc = v3; }
    });
    bool claimed = false;
    unsigned natom = 0;
    if (lead) {
        unsigned long long h = fuse_hash(key) & a.mask;
        FuseEntry *en = nullptr;
        for (unsigned s = 0; s < a.bound; s++, h = (h + 1) & a.mask) {
            // a long chain: stop once the insert is known to overflow (the flag is set by an atomic, polled by sc1 loads)
            if ((s & 63) == 63 && (__hip_atomic_load(&a.tot->abort, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ||
                                   fuse_overflowed(a.shards, a.max_voxels))) {
                atomicOr(&a.tot->abort, 1u);
                break;
            }
            unsigned long long cur = __hip_atomic_load(&a.table[h].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == kFuseEmpty) {
                cur = atomicCAS(&a.table[h].key, kFuseEmpty, key);
                natom++;
                if (cur == kFuseEmpty) { claimed = true; en = a.table + h; break; }
            }
            if (cur == key) { en = a.table + h; break; }
        }
        if (!en) {
            atomicOr(&a.tot->abort, 1u);      // bound reached (more than max_voxels distinct keys), or overflow seen above
        } else {
            atomicAdd(&en->count, cc & 0xFFu);
            atomicMin(&en->first, e);
            atomicAdd(&en->S[0], (unsigned long long)s0);
            atomicAdd(&en->S[1], (unsigned long long)s1);
            atomicAdd(&en->S[2], (unsigned long long)s2);
            natom += 5;
            if (a.color) { atomicAdd(&en->csum, (unsigned long long)(cc >> 8)); natom++; }
        }
    }
    const unsigned long long cl = __ballot(claimed);
    if (lane == 0 && cl) atomicAdd(&sh->claims, (unsigned)__popcll(cl));
    if (a.count_atomics) {
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) natom += __shfl_xor(natom, d);
        if (lane == 0 && natom) atomicAdd(&sh->atomics, (unsigned long long)natom);
    }
}

__global__ __launch_bounds__(kFuseBlock) void fuse_total_kernel(const FuseShard *__restrict__ shards, FuseTotals *__restrict__ tot)
{
    __shared__ unsigned long long part[3][kFuseBlock / 64];
    unsigned long long c = shards[threadIdx.x].claims, rj = shards[threadIdx.x].rejected, at = shards[threadIdx.x].atomics;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { c += __shfl_xor(c, d); rj += __shfl_xor(rj, d); at += __shfl_xor(at, d); }
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = c; part[1][threadIdx.x >> 6] = rj; part[2][threadIdx.x >> 6] = at; }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long s[3] = {0, 0, 0};
        for (int k = 0; k < 3; k++) for (int w = 0; w < kFuseBlock / 64; w++) s[k] += part[k][w];
        tot->ndist = s[0] > 0xFFFFFFFFull ? 0xFFFFFFFFu : (unsigned)s[0];
        tot->rejected = s[1];
        tot->atomics = s[2];
    }
}

__global__ __launch_bounds__(kFuseBlock) void fuse_flag_kernel(FuseArgs a, uint8_t *__restrict__ flags)
{
    const int lane = threadIdx.x & 63;
    const size_t e64 = (size_t)blockIdx.x * kFuseBlock + threadIdx.x;
    const unsigned e = (unsigned)e64;
    const bool fits = a.tot->ndist <= a.max_voxels;          // otherwise: SLR_ERR_OOM, nothing is flagged
    unsigned long long key = kFuseEmpty;
    unsigned q[3];
    bool ok = false;
    if (fits && e64 < a.n && a.has[e]) ok = fuse_key(a, e, &key, q);
    if (!ok) key = kFuseEmpty;
    uint8_t f = 0;
    bool lead = false;
    fuse_groups(ok, key, [&](bool, int l, unsigned long long) { lead |= lane == l; });
    if (lead) {                                      // only a group's leader can be its cell's first member
        const FuseEntry *en = fuse_find(a, key);
        f = en && en->first == e && en->count >= a.min_points;
    }
    if (e64 < a.n) flags[e64] = f;
}

__global__ __launch_bounds__(kFuseBlock) void fuse_emit_kernel(FuseArgs a, const uint32_t *__restrict__ src, const uint32_t *__restrict__ total,
                                                               float *__restrict__ out_xyz, uint32_t *__restrict__ out_count,
                                                               uint8_t *__restrict__ out_color)
{
    const unsigned m = *total < a.max_voxels ? *total : a.max_voxels;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.tot->emitted = m;
    for (size_t k = (size_t)blockIdx.x * kFuseBlock + threadIdx.x; k < m; k += (size_t)gridDim.x * kFuseBlock) {
        const unsigned e = src[k];
        unsigned long long key;
        unsigned q[3];
        if (!fuse_key(a, e, &key, q)) continue;                 // (cannot happen: e was flagged as a cell's first member)
        const FuseEntry *en = fuse_find(a, key);
        if (!en) continue;
        const unsigned long long c = en->count;
#pragma unroll
        for (int ax = 0; ax < 3; ax++) {
            const unsigned long long S = en->S[ax];
            const double v = (double)((long long)((key >> (21 * ax)) & 0x1FFFFFull) - (1ll << 20));
            const double frac = ((double)(S / c) + (double)(S % c) / (double)c) / kFuseQ;
            out_xyz[3 * k + ax] = (float)(a.org[ax] + (v + frac) * a.voxel);
        }
        out_count[k] = (uint32_t)c;
        if (out_color) out_color[k] = (uint8_t)((en->csum + c / 2) / c);
    }
}

hipError_t launch_fuse_voxels(const FuseLaunch &L, int phase, hipStream_t s)
{
    FuseArgs a;
    a.xyz = L.xyz; a.has = L.has; a.color = L.color; a.T = L.T;
    a.n = L.n; a.frame_px = L.frame_px;
    a.voxel = L.voxel; a.org[0] = L.origin[0]; a.org[1] = L.origin[1]; a.org[2] = L.origin[2];
    const size_t entries = fuse_table_entries(L.max_voxels);
    a.table = reinterpret_cast<FuseEntry *>(L.table); a.mask = entries - 1;
    a.bound = (unsigned)((size_t)L.max_voxels + 1 < entries ? (size_t)L.max_voxels + 1 : entries);
    a.max_voxels = L.max_voxels; a.min_points = L.min_points;
    a.shards = reinterpret_cast<FuseShard *>(L.stats);
    a.tot = reinterpret_cast<FuseTotals *>(reinterpret_cast<uint8_t *>(L.stats) + kFuseShards * sizeof(FuseShard));
    a.count_atomics = L.count_atomics;
    const size_t pgrid = (L.n + kFuseBlock - 1) / kFuseBlock;
    if (pgrid > 0x7fffffffu) return hipErrorInvalidValue;
    switch (phase) {
        case FUSE_CLEAR:
            SLR_LAUNCH(fuse_clear_kernel, dim3((unsigned)((entries + kFuseBlock - 1) / kFuseBlock)), dim3(kFuseBlock), 0, s, a.table, entries,
                       a.shards, a.tot);
            break;
        case FUSE_INSERT:
            if (pgrid) SLR_LAUNCH(fuse_insert_kernel, dim3((unsigned)pgrid), dim3(kFuseBlock), 0, s, a);
            break;
        case FUSE_TOTAL:
            SLR_LAUNCH(fuse_total_kernel, dim3(1), dim3(kFuseBlock), 0, s, (const FuseShard *)a.shards, a.tot);
            break;
        case FUSE_FLAG:
            if (pgrid) SLR_LAUNCH(fuse_flag_kernel, dim3((unsigned)pgrid), dim3(kFuseBlock), 0, s, a, L.flags);
            break;
        case FUSE_EMIT: {
            const size_t want = ((size_t)L.max_voxels + kFuseBlock - 1) / kFuseBlock;
            SLR_LAUNCH(fuse_emit_kernel, dim3((unsigned)(want < 4096 ? want : 4096)), dim3(kFuseBlock), 0, s, a, (const uint32_t *)L.src,
                       (const uint32_t *)L.total, L.out_xyz, L.out_count, L.out_color);
            break;
        }
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace slr

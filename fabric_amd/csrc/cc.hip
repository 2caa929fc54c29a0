// libbidate_hip: connected components of a scene mask -- label, compact, filter by area, per-object statistics.  The reference stops at the
// pixel mask of a scene (train.py:199); dropping speckle and counting objects would be scipy.ndimage.label + np.bincount on the host
// after a device-to-host copy of the mask.  Here the mask stays on the device:
//   bdn_cc_label    three launches: cc_tile_kernel labels each 64 x 64 tile in LDS (row runs from 64-bit row masks and bit scans, runs of
//                   neighbouring rows joined through an LDS union-find) and writes provisional global parents; cc_seam_kernel joins every
//                   tile-border pixel with its neighbours across the border; cc_flatten_kernel follows every pixel's chain to its root,
//                   writes the labels, adds the areas and counts.
//   bdn_cc_compact  four launches: root counts per block, one block scans the block counts, ranks at the roots, ranks spread to the rest.
//   bdn_cc_filter   one launch, bdn_cc_stats two (table initialisation, then integer atomics).
// The launch count depends on H and W only; nothing is read back.  Every union is the decreasing-parent form of cc_core.hpp: a parent only
// ever decreases, so a component's final root is its smallest linear index whatever the arrival order, and every sum is an integer sum:
// the outputs are the same bits on every run.  Every loop has a strictly decreasing quantity, stated where the loop is, and an iteration
// cap that raises counts[2]; no loop waits for another thread, wave or block.  No floating point anywhere in this file.
#include "common.hpp"
#include "cc_core.hpp"

constexpr int CC_THREADS = 256;
constexpr int CC_MAX_BLOCKS = 2048;                        // grid-strided kernels: 8 blocks per CU
constexpr long long CC_MAX_PIXELS = 2147483646LL;          // 2^31 - 2: 1 + (largest index) still fits an int32 label
constexpr int CC_TILE_CAP = CC_TILE * CC_TILE;             // iteration cap of the in-tile walks: a tile has that many nodes
constexpr int CC_SCAN_ITEMS = 4 * CC_THREADS;              // items per block of the compaction's prefix sum (4 per thread)

struct LdsPar {
    int* p;
    __device__ __forceinline__ int load(int i) const { return reinterpret_cast<volatile int*>(p)[i]; }
    __device__ __forceinline__ int fetch_min(int i, int v) { return atomicMin(&p[i], v); }
};
// Seam kernel: another XCD's block of the same launch may have written the parent, so every read is a relaxed agent-scope atomic load (a
// stale value is still an ancestor of the same set and costs iterations only) and every decision an atomicMin's return value.
struct GlobalPar {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int fetch_min(int i, int v) { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
// Flatten kernel: a later launch than every union, plain loads see the final parents.
struct PlainPar {
    const int* p;
    __device__ __forceinline__ int load(int i) const { return p[i]; }
};

template <int PER> struct IntVec;
template <> struct IntVec<1> {
    __device__ __forceinline__ static void load(const int* p, int* v) { v[0] = p[0]; }
    __device__ __forceinline__ static void store(int* p, const int* v) { p[0] = v[0]; }
    __device__ __forceinline__ static void bytes(const uint8_t* p, int* v) { v[0] = p[0]; }
    __device__ __forceinline__ static void store_bytes(uint8_t* p, const int* v) { p[0] = (uint8_t)v[0]; }
};
template <> struct IntVec<4> {
    __device__ __forceinline__ static void load(const int* p, int* v) {
        const int4 u = *reinterpret_cast<const int4*>(p);
        v[0] = u.x; v[1] = u.y; v[2] = u.z; v[3] = u.w;
    }
    __device__ __forceinline__ static void store(int* p, const int* v) { *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]); }
    __device__ __forceinline__ static void bytes(const uint8_t* p, int* v) {
        const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
        v[0] = u & 255; v[1] = u >> 8 & 255; v[2] = u >> 16 & 255; v[3] = u >> 24;
    }
    __device__ __forceinline__ static void store_bytes(uint8_t* p, const int* v) {
        *reinterpret_cast<uint32_t*>(p) = (uint32_t)v[0] | (uint32_t)v[1] << 8 | (uint32_t)v[2] << 16 | (uint32_t)v[3] << 24;
    }
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
    for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

static inline unsigned cc_grid(long long n_items) {
    const long long want = (n_items + CC_THREADS - 1) / CC_THREADS;
    return (unsigned)(want < 1 ? 1 : want < CC_MAX_BLOCKS ? want : CC_MAX_BLOCKS);
}

// ============================================================ workspace
// [parent: H W int32 | one status word per tile | the block counts of the compaction's prefix sum], each part padded to 16 bytes
struct CcLayout { long long HW; int tiles_y, tiles_x; long long n_tiles, n_scan; size_t off_status, off_scan, bytes; };
static inline size_t up16(size_t n) { return (n + 15) / 16 * 16; }
static inline bool cc_layout(int H, int W, CcLayout& L) {
    if (H < 1 || W < 1 || (long long)H * W > CC_MAX_PIXELS) return false;
    L.HW = (long long)H * W;
    L.tiles_y = (H + CC_TILE - 1) / CC_TILE; L.tiles_x = (W + CC_TILE - 1) / CC_TILE;
    L.n_tiles = (long long)L.tiles_y * L.tiles_x;
    L.n_scan = (L.HW + CC_SCAN_ITEMS - 1) / CC_SCAN_ITEMS;                   // the scalar path's block count, the larger one
    L.off_status = up16((size_t)L.HW * 4);
    L.off_scan = L.off_status + up16((size_t)L.n_tiles * 4);
    L.bytes = L.off_scan + up16((size_t)L.n_scan * 4);
    return true;
}

extern "C" size_t bdn_cc_workspace_bytes(int H, int W) {
    CcLayout L;
    return cc_layout(H, W, L) ? L.bytes : 0;
}

extern "C" int bdn_cc_tile(void) { return CC_TILE; }

// ============================================================ label: tiles
struct LabelArgs {
    const uint8_t* src; const uint8_t* excl; int* parent; int* area; int* counts; int* tile_status;
    int fg, exv, conn, H, W, tiles_x;
};

// One block per 64 x 64 tile, 256 threads, thread t owns the four pixels (row q >> 4, columns 4 (q & 15) ..) of q = t, t + 256, ...: with
// PER = 4 (W % 4 == 0, aligned pointers) one 4-byte load of src / exclude and one 16-byte store of the parents and of the area zeros per
// quad; PER = 1: single bytes and words, bounds-checked per pixel.  Pixels outside the raster are background and are not written.
template <int PER>
__global__ __launch_bounds__(CC_THREADS) void cc_tile_kernel(const LabelArgs a) {
    __shared__ unsigned rowbits[CC_TILE][2];               // row r's foreground mask, bit c = column c of the tile
    __shared__ int lp[CC_TILE * CC_TILE];                  // local parents, node = 64 r + c
    __shared__ int st_lds;
    const int tid = threadIdx.x;
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int y0 = ty * CC_TILE, x0 = tx * CC_TILE;
    if (blockIdx.x == 0 && tid < 4) a.counts[tid] = 0;     // the later launches add into them
    if (tid < 2 * CC_TILE) (&rowbits[0][0])[tid] = 0;
    if (tid == 0) st_lds = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = tid + CC_THREADS * k, r = q >> 4, c4 = (q & 15) * 4;
        const int y = y0 + r, x = x0 + c4;
        unsigned nib = 0;
        if (y < a.H && x < a.W) {
            const size_t at = (size_t)y * a.W + x;
            if constexpr (PER == 4) {                      // W % 4 == 0 and x % 4 == 0: the quad is inside
                int s[4], e[4] = {0, 0, 0, 0};
                IntVec<4>::bytes(a.src + at, s);
                if (a.excl) IntVec<4>::bytes(a.excl + at, e);
#pragma unroll
                for (int j = 0; j < 4; j++) nib |= (unsigned)(s[j] == a.fg && !(a.excl && e[j] == a.exv)) << j;
            } else {
                for (int j = 0; j < 4 && x + j < a.W; j++)
                    nib |= (unsigned)(a.src[at + j] == a.fg && !(a.excl && a.excl[at + j] == a.exv)) << j;
            }
        }
        if (nib) atomicOr(&rowbits[r][c4 >> 5], nib << (c4 & 31));
    }
    __syncthreads();
    // every pixel of a run starts under the run's first pixel
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = tid + CC_THREADS * k, r = q >> 4, c4 = (q & 15) * 4;
        const uint64_t m = (uint64_t)rowbits[r][0] | (uint64_t)rowbits[r][1] << 32;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = c4 + j;
            lp[r * CC_TILE + c] = r * CC_TILE + ((m >> c & 1) ? cc_run_start(m, c) : c);
        }
    }
    __syncthreads();
    // runs of neighbouring rows: cc_links picks one link per pair of touching runs, cc_union joins them (bounded, see cc_core.hpp)
    LdsPar par{lp};
    int status = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = tid + CC_THREADS * k, r = q >> 4, c4 = (q & 15) * 4;
        if (r == 0) continue;
        const uint64_t m = (uint64_t)rowbits[r][0] | (uint64_t)rowbits[r][1] << 32;
        const uint64_t mu = (uint64_t)rowbits[r - 1][0] | (uint64_t)rowbits[r - 1][1] << 32;
        if (!(m >> c4 & 15) || !mu) continue;
        for (int j = 0; j < 4; j++) {
            const int c = c4 + j;
            const int links = cc_links(m, mu, c, CC_TILE, a.conn);
            for (int d = 0; d < 3; d++)
                if (links >> d & 1)
                    cc_union(par, r * CC_TILE + cc_run_start(m, c), (r - 1) * CC_TILE + cc_run_start(mu, c + d - 1), CC_TILE_CAP, &status);
        }
    }
    __syncthreads();
    // the tile's roots are its smallest local nodes, and local order is global order inside a tile: parent = the root's linear index
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int q = tid + CC_THREADS * k, r = q >> 4, c4 = (q & 15) * 4;
        const int y = y0 + r, x = x0 + c4;
        if (y >= a.H || x >= a.W) continue;
        const uint64_t m = (uint64_t)rowbits[r][0] | (uint64_t)rowbits[r][1] << 32;
        int g[4];
        const int zero[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            g[j] = -1;
            if (m >> (c4 + j) & 1) {
                const int root = cc_find(par, r * CC_TILE + c4 + j, CC_TILE_CAP, &status);
                g[j] = (y0 + (root >> 6)) * a.W + x0 + (root & 63);
            }
        }
        const size_t at = (size_t)y * a.W + x;
        if constexpr (PER == 4) {
            IntVec<4>::store(a.parent + at, g);
            if (a.area) IntVec<4>::store(a.area + at, zero);
        } else {
            for (int j = 0; j < 4 && x + j < a.W; j++) {
                a.parent[at + j] = g[j];
                if (a.area) a.area[at + j] = 0;
            }
        }
    }
    if (status) st_lds = 1;
    __syncthreads();
    if (tid == 0) a.tile_status[blockIdx.x] = st_lds;
}

// ============================================================ label: seams
// One thread per pixel of the first row of every tile row but the top one (it looks across the border at the row above) and of the first
// column of every tile column but the left one (it looks at the column to the left).  With 8-connectivity the two diagonals across the
// border are among the links, the ones at a four-tile corner included.  Foreground is parent >= 0, which no launch after the tiles changes.
// cc_links drops a link when the column before it makes the same one, which needs the two pixels of this side joined already: true
// inside a tile only, so a neighbour along the seam that lies in another tile is left out of this side's mask (the link is then made).
__global__ __launch_bounds__(CC_THREADS) void cc_seam_kernel(int* parent, int* counts, int H, int W, int conn, long long n_h, long long total, int cap) {
    GlobalPar par{parent};
    int status = 0;
    const long long stride = (long long)gridDim.x * CC_THREADS;
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < total; i += stride) {
        int y, x, dy, dx, lim, pos;                       // (dy, dx): the step along the seam; pos in [0, lim): the place along it
        if (i < n_h) {
            const int s = (int)(i / W);
            x = (int)(i - (long long)s * W); y = (s + 1) * CC_TILE; dy = 0; dx = 1; lim = W; pos = x;
        } else {
            const long long j = i - n_h;
            const int s = (int)(j / H);
            y = (int)(j - (long long)s * H); x = (s + 1) * CC_TILE; dy = 1; dx = 0; lim = H; pos = y;
        }
        const int cur = y * W + x;
        if (par.load(cur) < 0) continue;
        const int oy = y - dx, ox = x - dy;               // the pixel across the border
        unsigned m = 2, mu = 0;
#pragma unroll
        for (int d = -1; d <= 1; d++) {
            if (pos + d < 0 || pos + d >= lim) continue;
            if (d && (pos + d) / CC_TILE == pos / CC_TILE && par.load((y + d * dy) * W + x + d * dx) >= 0) m |= 1u << (d + 1);
            if (par.load((oy + d * dy) * W + ox + d * dx) >= 0) mu |= 1u << (d + 1);
        }
        const int links = cc_links(m, mu, 1, 3, conn);
        for (int d = 0; d < 3; d++)
            if (links >> d & 1) cc_union(par, cur, (oy + (d - 1) * dy) * W + ox + (d - 1) * dx, cap, &status);
    }
    if (status) atomicOr(&counts[2], 1);
}

// ============================================================ label: flatten
// One add of the wave's pixels into area[root].  key = the pixel's root, or < 0 for a lane without a foreground pixel.  As wave_hist_add
// of curve.hip: twice, the lanes that share the key of the first pending lane are counted by a ballot and added once; the rest add singly.
// Must be called by all 64 lanes of the wave together.
__device__ __forceinline__ void wave_root_add(int* area, int key, int lane) {
    bool pending = key >= 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const unsigned long long act = __ballot(pending);
        if (!act) return;                                  // wave-uniform
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
        const int k = __builtin_amdgcn_readlane(key, leader);
        const bool mine = pending && key == k;
        const unsigned long long same = __ballot(mine);
        if (lane == leader) atomicAdd(&area[k], __popcll(same));
        pending = pending && !mine;
    }
    if (pending) atomicAdd(&area[key], 1);
}

// An item is PER consecutive pixels.  The trip count is the same for every thread of a block (the ballots need whole waves).
template <int PER>
__global__ __launch_bounds__(CC_THREADS) void cc_flatten_kernel(const int* __restrict__ parent, int* __restrict__ labels, int* area, int* counts,
                                                                const int* __restrict__ tile_status, long long n_tiles, long long n_items, int cap) {
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    PlainPar par{parent};
    int status = 0, n_root = 0, n_fg = 0;
    const long long stride = (long long)gridDim.x * CC_THREADS, base0 = (long long)blockIdx.x * CC_THREADS;
    for (long long t = base0 + tid; t < n_tiles; t += stride) status |= tile_status[t];
    for (long long base = base0; base < n_items; base += stride) {
        const long long it = base + tid;
        int root[PER];
#pragma unroll
        for (int j = 0; j < PER; j++) root[j] = -1;
        if (it < n_items) {
            int p[PER], lab[PER];
            IntVec<PER>::load(parent + it * PER, p);
#pragma unroll
            for (int j = 0; j < PER; j++) {
                lab[j] = 0;
                if (p[j] >= 0) {
                    root[j] = cc_find(par, p[j], cap, &status);         // the node strictly decreases along the chain
                    lab[j] = root[j] + 1;
                    n_fg++;
                    n_root += root[j] == (int)(it * PER + j);
                }
            }
            IntVec<PER>::store(labels + it * PER, lab);
        }
        if (area) {
#pragma unroll
            for (int j = 0; j < PER; j++) wave_root_add(area, root[j], lane);
        }
    }
    n_root = wave_sum(n_root); n_fg = wave_sum(n_fg);
    if (lane == 0) { atomicAdd(&s_cnt[0], n_root); atomicAdd(&s_cnt[1], n_fg); }
    __syncthreads();
    if (tid < 2 && s_cnt[tid]) atomicAdd(&counts[tid], s_cnt[tid]);          // one integer add per block and counter
    if (status) atomicOr(&counts[2], 1);
}

static inline bool al(const void* p, uintptr_t a) { return (uintptr_t)p % a == 0; }

extern "C" int bdn_cc_label(const uint8_t* src, int fg_value, const uint8_t* exclude, int exclude_value, int connectivity, int H, int W,
                            int32_t* labels, int32_t* area, int32_t* counts, void* workspace, void* stream) {
    if (!src || !labels || !counts || !workspace) BDN_FAIL(BDN_E_ARG, "cc_label: null pointer");
    if (!al(labels, 4) || !al(area, 4) || !al(counts, 4) || !al(workspace, 16))
        BDN_FAIL(BDN_E_ARG, "cc_label: labels / area / counts must be 4-byte, workspace 16-byte aligned");
    if (connectivity != 4 && connectivity != 8) BDN_FAIL(BDN_E_ARG, "cc_label: connectivity must be 4 or 8, got %d", connectivity);
    if (fg_value < 0 || fg_value > 255) BDN_FAIL(BDN_E_ARG, "cc_label: fg_value must be a byte 0..255, got %d", fg_value);
    if (exclude && (exclude_value < 0 || exclude_value > 255)) BDN_FAIL(BDN_E_ARG, "cc_label: exclude_value must be a byte 0..255, got %d", exclude_value);
    CcLayout L;
    if (!cc_layout(H, W, L)) BDN_FAIL(BDN_E_ARG, "cc_label: need 1 <= H, W and H * W <= 2^31 - 2, got %d x %d", H, W);
    char* ws = (char*)workspace;
    LabelArgs a;
    a.src = src; a.excl = exclude; a.parent = (int*)ws; a.area = area; a.counts = counts; a.tile_status = (int*)(ws + L.off_status);
    a.fg = fg_value; a.exv = exclude_value; a.conn = connectivity; a.H = H; a.W = W; a.tiles_x = L.tiles_x;
    const bool vec = W % 4 == 0 && al(src, 4) && al(exclude, 4) && al(labels, 16) && al(area, 16);
    const int cap = (int)L.HW;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(cc_tile_kernel<4>, dim3((unsigned)L.n_tiles), dim3(CC_THREADS), 0, st, a);
    else hipLaunchKernelGGL(cc_tile_kernel<1>, dim3((unsigned)L.n_tiles), dim3(CC_THREADS), 0, st, a);
    BDN_CHECK_LAUNCH("cc_label (tiles)");
    const long long n_h = (long long)(L.tiles_y - 1) * W, total = n_h + (long long)(L.tiles_x - 1) * H;
    if (total > 0) {                                       // a function of H and W only
        hipLaunchKernelGGL(cc_seam_kernel, dim3(cc_grid(total)), dim3(CC_THREADS), 0, st, a.parent, counts, H, W, connectivity, n_h, total, cap);
        BDN_CHECK_LAUNCH("cc_label (seams)");
    }
    const long long n_items = vec ? L.HW / 4 : L.HW;
    if (vec) hipLaunchKernelGGL(cc_flatten_kernel<4>, dim3(cc_grid(n_items)), dim3(CC_THREADS), 0, st, a.parent, labels, area, counts, a.tile_status, L.n_tiles, n_items, cap);
    else hipLaunchKernelGGL(cc_flatten_kernel<1>, dim3(cc_grid(n_items)), dim3(CC_THREADS), 0, st, a.parent, labels, area, counts, a.tile_status, L.n_tiles, n_items, cap);
    BDN_CHECK_LAUNCH("cc_label (flatten)");
    return BDN_OK;
}

// ============================================================ compact
// A root is a pixel whose label is 1 + its own index.  Block b owns the items [b CC_SCAN_ITEMS, (b + 1) CC_SCAN_ITEMS), wave w of it a
// quarter, in four steps of 64 consecutive items.  Fixed passes: no block waits for another.
template <int PER> __device__ __forceinline__ int root_flags(const int* labels, long long it, long long n_items, int* lab) {
    int f = 0;
#pragma unroll
    for (int j = 0; j < PER; j++) lab[j] = 0;
    if (it < n_items) {
        IntVec<PER>::load(labels + it * PER, lab);
#pragma unroll
        for (int j = 0; j < PER; j++) f |= (lab[j] == (int)(it * PER + j) + 1) << j;
    }
    return f;
}

template <int PER>
__global__ __launch_bounds__(CC_THREADS) void cc_rootsum_kernel(const int* __restrict__ labels, long long n_items, int* __restrict__ sums) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long w0 = (long long)blockIdx.x * CC_SCAN_ITEMS + wave * 256;
    int n = 0, lab[PER];
#pragma unroll
    for (int k = 0; k < 4; k++) n += __popc(root_flags<PER>(labels, w0 + k * 64 + lane, n_items, lab));
    n = wave_sum(n);
    if (lane == 0) s_w[wave] = n;
    __syncthreads();
    if (tid == 0) sums[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// One block: sums[0..nb) becomes its exclusive prefix sum, the total goes to counts[0].  Thread t owns a contiguous stretch.
__global__ __launch_bounds__(1024) void cc_scan_kernel(int* sums, long long nb, int* counts) {
    __shared__ int s_t[1024];
    const int t = threadIdx.x;
    const long long per = (nb + 1023) / 1024, lo = t * per, hi = lo + per < nb ? lo + per : nb;
    int s = 0;
    for (long long i = lo; i < hi; i++) s += sums[i];
    s_t[t] = s;
    __syncthreads();
    int before = 0;
    for (int k = 0; k < t; k++) before += s_t[k];
    for (long long i = lo; i < hi; i++) { const int v = sums[i]; sums[i] = before; before += v; }
    if (t == 1023 && counts) counts[0] = before;
}

// compact = the 1-based rank at a root, 0 elsewhere (background for good, the other foreground pixels until cc_spread_kernel).
template <int PER>
__global__ __launch_bounds__(CC_THREADS) void cc_rank_kernel(const int* __restrict__ labels, long long n_items, const int* __restrict__ sums, int* __restrict__ compact) {
    __shared__ int s_w[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long w0 = (long long)blockIdx.x * CC_SCAN_ITEMS + wave * 256;
    int n = 0, lab[PER];
#pragma unroll
    for (int k = 0; k < 4; k++) n += __popc(root_flags<PER>(labels, w0 + k * 64 + lane, n_items, lab));
    n = wave_sum(n);
    if (lane == 0) s_w[wave] = n;
    __syncthreads();
    int base = sums[blockIdx.x];
    for (int w = 0; w < wave; w++) base += s_w[w];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const long long it = w0 + k * 64 + lane;
        const int f = root_flags<PER>(labels, it, n_items, lab), c = __popc(f);
        int incl = c;                                      // inclusive prefix over the lanes
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(incl, o); if (lane >= o) incl += v; }
        int rank = base + incl - c, out[PER];
#pragma unroll
        for (int j = 0; j < PER; j++) { out[j] = 0; if (f >> j & 1) out[j] = ++rank; }
        if (it < n_items) IntVec<PER>::store(compact + it * PER, out);
        base += __shfl(incl, 63);
    }
}

// Every foreground pixel that is no root takes its root's rank.  Roots are not written here, so every rank read is final.
__global__ __launch_bounds__(CC_THREADS) void cc_spread_kernel(const int* __restrict__ labels, long long n, int* compact) {
    const long long stride = (long long)gridDim.x * CC_THREADS;
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += stride) {
        const int l = labels[i];
        if (l != 0 && l != (int)i + 1) compact[i] = compact[l - 1];
    }
}

extern "C" int bdn_cc_compact(const int32_t* labels, int H, int W, int32_t* compact, int32_t* counts, void* workspace, void* stream) {
    if (!labels || !compact || !workspace) BDN_FAIL(BDN_E_ARG, "cc_compact: null pointer");
    if (!al(labels, 4) || !al(compact, 4) || !al(counts, 4) || !al(workspace, 16))
        BDN_FAIL(BDN_E_ARG, "cc_compact: labels / compact / counts must be 4-byte, workspace 16-byte aligned");
    if (labels == compact) BDN_FAIL(BDN_E_ARG, "cc_compact: compact must not alias labels");
    CcLayout L;
    if (!cc_layout(H, W, L)) BDN_FAIL(BDN_E_ARG, "cc_compact: need 1 <= H, W and H * W <= 2^31 - 2, got %d x %d", H, W);
    int* sums = (int*)((char*)workspace + L.off_scan);
    const bool vec = W % 4 == 0 && al(labels, 16) && al(compact, 16);
    const long long n_items = vec ? L.HW / 4 : L.HW, nb = (n_items + CC_SCAN_ITEMS - 1) / CC_SCAN_ITEMS;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(cc_rootsum_kernel<4>, dim3((unsigned)nb), dim3(CC_THREADS), 0, st, labels, n_items, sums);
    else hipLaunchKernelGGL(cc_rootsum_kernel<1>, dim3((unsigned)nb), dim3(CC_THREADS), 0, st, labels, n_items, sums);
    BDN_CHECK_LAUNCH("cc_compact (block sums)");
    hipLaunchKernelGGL(cc_scan_kernel, dim3(1), dim3(1024), 0, st, sums, nb, counts);
    BDN_CHECK_LAUNCH("cc_compact (scan)");
    if (vec) hipLaunchKernelGGL(cc_rank_kernel<4>, dim3((unsigned)nb), dim3(CC_THREADS), 0, st, labels, n_items, sums, compact);
    else hipLaunchKernelGGL(cc_rank_kernel<1>, dim3((unsigned)nb), dim3(CC_THREADS), 0, st, labels, n_items, sums, compact);
    BDN_CHECK_LAUNCH("cc_compact (ranks)");
    hipLaunchKernelGGL(cc_spread_kernel, dim3(cc_grid(L.HW)), dim3(CC_THREADS), 0, st, labels, L.HW, compact);
    BDN_CHECK_LAUNCH("cc_compact (spread)");
    return BDN_OK;
}

// ============================================================ filter
template <int PER>
__global__ __launch_bounds__(CC_THREADS) void cc_filter_kernel(const int* __restrict__ labels, const int* __restrict__ area, int min_area, uint8_t* out, long long n_items) {
    const long long stride = (long long)gridDim.x * CC_THREADS;
    for (long long it = (long long)blockIdx.x * CC_THREADS + threadIdx.x; it < n_items; it += stride) {
        int lab[PER], keep[PER];
        IntVec<PER>::load(labels + it * PER, lab);
#pragma unroll
        for (int j = 0; j < PER; j++) keep[j] = lab[j] != 0 && (min_area <= 1 || area[lab[j] - 1] >= min_area);
        IntVec<PER>::store_bytes(out + it * PER, keep);
    }
}

extern "C" int bdn_cc_filter(const uint8_t* src_mask, const int32_t* labels, const int32_t* area, int min_area, uint8_t* out_mask, int H, int W,
                             void* stream) {
    (void)src_mask;                                        // the labels carry the foreground test and the exclusion; never dereferenced
    if (!labels || !out_mask || (!area && min_area > 1)) BDN_FAIL(BDN_E_ARG, "cc_filter: null pointer");
    if (!al(labels, 4) || !al(area, 4)) BDN_FAIL(BDN_E_ARG, "cc_filter: labels / area must be 4-byte aligned");
    if (H < 1 || W < 1 || (long long)H * W > CC_MAX_PIXELS) BDN_FAIL(BDN_E_ARG, "cc_filter: need 1 <= H, W and H * W <= 2^31 - 2, got %d x %d", H, W);
    const long long HW = (long long)H * W;
    const bool vec = W % 4 == 0 && al(labels, 16) && al(out_mask, 4);
    const long long n_items = vec ? HW / 4 : HW;
    hipStream_t st = (hipStream_t)stream;
    if (vec) hipLaunchKernelGGL(cc_filter_kernel<4>, dim3(cc_grid(n_items)), dim3(CC_THREADS), 0, st, labels, area, min_area, out_mask, n_items);
    else hipLaunchKernelGGL(cc_filter_kernel<1>, dim3(cc_grid(n_items)), dim3(CC_THREADS), 0, st, labels, area, min_area, out_mask, n_items);
    BDN_CHECK_LAUNCH("cc_filter");
    return BDN_OK;
}

// ============================================================ stats
__global__ __launch_bounds__(CC_THREADS) void cc_stats_init_kernel(int* table, int n_max, int H, int W) {
    const long long n = (long long)n_max * 8, stride = (long long)gridDim.x * CC_THREADS;
    for (long long i = (long long)blockIdx.x * CC_THREADS + threadIdx.x; i < n; i += stride) {
        const int c = (int)(i & 7);
        table[i] = c == 1 ? H : c == 2 ? W : c == 3 || c == 4 ? -1 : 0;
    }
}

// One pixel of every lane into the table.  key = compact label - 1, or < 0 for a lane with nothing to add.  Twice, the lanes that share
// the first pending lane's key are reduced in the wave (count by ballot, box by shuffles) and their leader adds once; the rest add singly.
// Must be called by all 64 lanes of the wave together.
__device__ __forceinline__ void wave_stats_add(int* table, int key, int y, int x, bool ov, int lane) {
    bool pending = key >= 0;
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const unsigned long long act = __ballot(pending);
        if (!act) return;                                  // wave-uniform
        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)act) - 1);
        const int k = __builtin_amdgcn_readlane(key, leader);
        const bool mine = pending && key == k;
        const int n = __popcll(__ballot(mine)), no = __popcll(__ballot(mine && ov));
        const int y0 = wave_min(mine ? y : 0x7fffffff), x0 = wave_min(mine ? x : 0x7fffffff);
        const int y1 = wave_max(mine ? y : -1), x1 = wave_max(mine ? x : -1);
        if (lane == leader) {
            int* row = table + (size_t)k * 8;
            atomicAdd(row, n); atomicMin(row + 1, y0); atomicMin(row + 2, x0); atomicMax(row + 3, y1); atomicMax(row + 4, x1);
            if (no) atomicAdd(row + 5, no);
        }
        pending = pending && !mine;
    }
    if (pending) {
        int* row = table + (size_t)key * 8;
        atomicAdd(row, 1); atomicMin(row + 1, y); atomicMin(row + 2, x); atomicMax(row + 3, y); atomicMax(row + 4, x);
        if (ov) atomicAdd(row + 5, 1);
    }
}

template <int PER>
__global__ __launch_bounds__(CC_THREADS) void cc_stats_kernel(const int* __restrict__ compact, int n_max, const uint8_t* __restrict__ other, int other_value,
                                                              int other_excl, int W, int* table, long long n_items) {
    const int tid = threadIdx.x, lane = tid & 63;
    const long long stride = (long long)gridDim.x * CC_THREADS, base0 = (long long)blockIdx.x * CC_THREADS;
    for (long long base = base0; base < n_items; base += stride) {      // the same trip count for every thread of a block
        const long long it = base + tid;
        int key[PER], o[PER], y = 0, x = 0;
#pragma unroll
        for (int j = 0; j < PER; j++) { key[j] = -1; o[j] = -1; }
        if (it < n_items) {
            int k[PER];
            IntVec<PER>::load(compact + it * PER, k);
            if (other) IntVec<PER>::bytes(other + it * PER, o);
            y = (int)(it * PER / W); x = (int)(it * PER - (long long)y * W);      // PER = 4: W % 4 == 0, the item lies in one row
#pragma unroll
            for (int j = 0; j < PER; j++)
                if (k[j] >= 1 && k[j] <= n_max && !(other && o[j] == other_excl)) key[j] = k[j] - 1;
        }
#pragma unroll
        for (int j = 0; j < PER; j++) wave_stats_add(table, key[j], y, x + j, other && o[j] == other_value, lane);
    }
}

extern "C" int bdn_cc_stats(const int32_t* compact, int n_max, const uint8_t* other, int other_value, int other_exclude_value, int H, int W,
                            int32_t* table, void* stream) {
    if (!compact || !table) BDN_FAIL(BDN_E_ARG, "cc_stats: null pointer");
    if (!al(compact, 4) || !al(table, 4)) BDN_FAIL(BDN_E_ARG, "cc_stats: compact / table must be 4-byte aligned");
    if (n_max < 1 || n_max > (1 << 28) - 1) BDN_FAIL(BDN_E_ARG, "cc_stats: n_max must be in 1..2^28 - 1, got %d", n_max);
    if (other && (other_value < 0 || other_value > 255)) BDN_FAIL(BDN_E_ARG, "cc_stats: other_value must be a byte 0..255, got %d", other_value);
    if (other && (other_exclude_value < -1 || other_exclude_value > 255))
        BDN_FAIL(BDN_E_ARG, "cc_stats: other_exclude_value must be -1 (none) or a byte 0..255, got %d", other_exclude_value);
    if (H < 1 || W < 1 || (long long)H * W > CC_MAX_PIXELS) BDN_FAIL(BDN_E_ARG, "cc_stats: need 1 <= H, W and H * W <= 2^31 - 2, got %d x %d", H, W);
    const long long HW = (long long)H * W;
    const bool vec = W % 4 == 0 && al(compact, 16) && al(other, 4);
    const long long n_items = vec ? HW / 4 : HW;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cc_stats_init_kernel, dim3(cc_grid((long long)n_max * 8)), dim3(CC_THREADS), 0, st, table, n_max, H, W);
    BDN_CHECK_LAUNCH("cc_stats (init)");
    if (vec) hipLaunchKernelGGL(cc_stats_kernel<4>, dim3(cc_grid(n_items)), dim3(CC_THREADS), 0, st, compact, n_max, other, other_value, other_exclude_value, W, table, n_items);
    else hipLaunchKernelGGL(cc_stats_kernel<1>, dim3(cc_grid(n_items)), dim3(CC_THREADS), 0, st, compact, n_max, other, other_value, other_exclude_value, W, table, n_items);
    BDN_CHECK_LAUNCH("cc_stats");
    return BDN_OK;
}

// Single-linkage clustering of the gallery at a similarity threshold (frt_matcher_cluster) for gfx950: the connected components
// of the graph "S(i, j) >= t", S being the exact fp32 similarity of the scans in kernels_match.hip.
//
// The host walks the gallery in chunks of 128 rows used as queries.  A chunk either goes through the screen - coarse scan and
// absolute-threshold selection (kernels_match.hip), then cluster_rerank_union_kernel over the listed (query, tile) pairs - or through the
// dense pass: match_kernel's full matrix of the chunk, then cluster_dense_union_kernel.  Both recompute / read S with the bits of the exact
// scan and unite every pair (i, j > i) with S >= t; no edge is stored.
//
// Union-find.  parent[N] with parent[x] <= x at all times: a root is the smallest row of its tree, so the final label of a component - the
// root - is its smallest row whatever order the device worked in.  unite(a, b) finds both roots and hooks the LARGER under the smaller with
// one compare-and-swap on the larger root's own slot (expected value = itself: only a root is ever hooked, and only once).  Every access to
// parent inside the union kernels is an agent-scope atomic: the L2 of an XCD is not coherent with the other XCDs' and a CU's L1 is never
// refreshed by another CU's stores, so a plain load may return a stale line for as long as the kernel runs - a plain re-read after a failed
// CAS could spin on it.  The loop instead continues from the value the failed CAS returned.  The one shortcut written back is
// atomicMin(parent[start], root): it can only replace an ancestor by a farther ancestor of the same tree, so parent[x] <= x and "x and
// parent[x] are in one component" keep holding; there is no path compression with plain stores.
#include <limits.h>

#include "frt_kernels.h"

namespace {

__device__ __forceinline__ int uf_load(int32_t *parent, int x) { return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_root(int32_t *parent, int x) {
    int p = uf_load(parent, x);
    while (p != x) {  // parent values only ever decrease and are bounded by 0: the walk ends
        x = p;
        p = uf_load(parent, x);
    }
    return x;
}

__device__ void uf_unite(int32_t *parent, int a, int b) {
    int ra = uf_root(parent, a), rb = uf_root(parent, b);
    while (ra != rb) {
        if (ra > rb) {
            const int t = ra;
            ra = rb;
            rb = t;
        }
        // rb > ra: hook rb under ra if rb is still a root
        int seen = rb;
        if (__hip_atomic_compare_exchange_strong(parent + rb, &seen, ra, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
        rb = uf_root(parent, seen);  // somebody hooked rb first, under `seen` < rb: go on from there
        ra = uf_root(parent, ra);
    }
    // both rows now hang under min(ra, rb) = ra or an ancestor of it; shorten their own first step
    const int r = ra < rb ? ra : rb;
    if (a != r) __hip_atomic_fetch_min(parent + a, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b != r) __hip_atomic_fetch_min(parent + b, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// one 64-bit atomic per wave: the number of lanes with `hit`
__device__ __forceinline__ void count_hits(bool hit, unsigned long long *counter) {
    const unsigned long long bal = __ballot(hit);
    if (bal && (int)(threadIdx.x & 63) == __ffsll((long long)bal) - 1) atomicAdd(counter, (unsigned long long)__popcll(bal));
}

__global__ __launch_bounds__(256) void cluster_init_kernel(int32_t *__restrict__ parent, int N, long long *__restrict__ stats) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) parent[i] = i;
    if (i < 4) stats[i] = 0;
}

// fragment-ordered fp16 rows -> fp32 row-major; thread = four columns of one row
__global__ __launch_bounds__(256) void cluster_queries_kernel(const half_t *__restrict__ G, int row0, int n, int D, float *__restrict__ out) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = D >> 2;
    const long r = t / per;
    if (r >= n) return;
    const int k = (int)(t - r * per) * 4;
    *reinterpret_cast<floatx4 *>(out + r * D + k) = load_g4(G, row0 + r, D, k);
}

// match_rerank_pairs_kernel with a join in place of the maximum: one workgroup (128 threads = the tile's 128 rows) per pair, the same k
// order and one fmaf per term, so that S has the bits of the exact scan.  Query q of the list is gallery row q_row0 + q; the list's tile
// numbers count from tile_origin (the coarse scan and the selection may have begun there: no row in front of the chunk is ever joined to
// it), G and N are the whole gallery.
template <typename GT>
__global__ __launch_bounds__(128) void cluster_rerank_union_kernel(const GT *__restrict__ G, int N, int D, const float *__restrict__ E, int q_row0,
                                                                   int tile_origin, const MatchPair *__restrict__ pairs, int pair_cap, const int *__restrict__ ctl, float thr,
                                                                   int32_t *__restrict__ parent, unsigned long long *__restrict__ edges,
                                                                   int *__restrict__ chunk_overflow) {
    extern __shared__ __attribute__((aligned(16))) char smem_c[];
    float *qs = reinterpret_cast<float *>(smem_c);  // [D]
    const int tid = threadIdx.x;
    const int overflow = ctl[FRT_MATCH_CTL_OVERFLOW];  // (final: the selection finished before this launch began)
    if (blockIdx.x == 0 && tid == 0) *chunk_overflow = overflow;
    if (overflow) return;  // the host runs this chunk through the dense pass: nothing is joined or counted twice
    const int sub_cap = pair_cap / FRT_MATCH_SEL_SUB;
    int maxc = 0;
    for (int sgi = 0; sgi < FRT_MATCH_SEL_SUB; ++sgi) maxc = max(maxc, min(ctl[FRT_MATCH_CTL_SEG0 + sgi * FRT_MATCH_CTL_STRIDE], sub_cap));
    for (int p = blockIdx.x; p < maxc * FRT_MATCH_SEL_SUB; p += gridDim.x) {  // virtual index over the sub-lists, interleaved
        const int sgi = p % FRT_MATCH_SEL_SUB, pi_ = p / FRT_MATCH_SEL_SUB;
        if (pi_ >= ctl[FRT_MATCH_CTL_SEG0 + sgi * FRT_MATCH_CTL_STRIDE]) continue;  // (block-uniform)
        const MatchPair pr = pairs[sgi * sub_cap + pi_];
        __syncthreads();  // the previous pair's readers of qs are done
        for (int k = tid * 4; k < D; k += 512) *reinterpret_cast<floatx4 *>(qs + k) = *reinterpret_cast<const floatx4 *>(E + (long)pr.q * D + k);
        __syncthreads();
        const int i = q_row0 + pr.q;
        const long g = ((long)tile_origin + (pr.tile & FRT_MATCH_PAIR_TILE_MASK)) * 128 + tid;
        // this row's 32-row block is inside the band, and the row comes after the query's own (i < j; never a row with itself)
        const bool live = g < N && g > i && ((((unsigned)pr.tile >> 28) >> (tid >> 5)) & 1u);
        float acc = 0.f;
        if (live) acc = exact_row_dot(G, g, D, qs);  // the exact kernel's k order, one fused multiply-add per term (frt_kernels.h)
        const bool hit = live && acc >= thr;  // (a NaN similarity joins nothing)
        if (hit) uf_unite(parent, i, (int)g);
        count_hits(hit, edges);
    }
}

// full [F][N]: row q = the exact similarities of gallery row q_row0 + q with every row.  Grid-stride over whole waves of 64 columns.
__global__ __launch_bounds__(256) void cluster_dense_union_kernel(const float *__restrict__ full, int F, int N, int q_row0, float thr,
                                                                  int32_t *__restrict__ parent, unsigned long long *__restrict__ edges) {
    const long cols = ((long)N + 63) / 64 * 64;  // (whole waves reach the ballot)
    const long total = (long)F * cols;
    for (long e0 = (long)blockIdx.x * 256; e0 < total; e0 += (long)gridDim.x * 256) {
        const long e = e0 + threadIdx.x;
        const int q = (int)(e / cols);
        const long j = e - (long)q * cols;
        const int i = q_row0 + q;
        bool hit = false;
        if (q < F && j < N && j > i) hit = full[(long)q * N + j] >= thr;
        if (hit) uf_unite(parent, i, (int)j);
        count_hits(hit, edges);
    }
}

// a launch of its own behind the last union: every store of the union kernels is visible, plain loads do
__global__ __launch_bounds__(256) void cluster_flatten_kernel(const int32_t *__restrict__ parent, int N, int32_t *__restrict__ labels,
                                                              long long *__restrict__ stats, long long screened_chunks, long long dense_chunks) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    bool root = false;
    if (i < N) {
        int x = i, p = parent[x];
        while (p != x) {
            x = p;
            p = parent[x];
        }
        labels[i] = x;
        root = x == i;
    }
    count_hits(root, reinterpret_cast<unsigned long long *>(stats));
    if (i == 0) {
        stats[2] = screened_chunks;
        stats[3] = dense_chunks;
    }
}

}  // namespace

void launch_cluster_init(int32_t *parent, int N, long long *stats, hipStream_t s) {
    hipLaunchKernelGGL(cluster_init_kernel, dim3((N + 255) / 256 > 0 ? (N + 255) / 256 : 1), dim3(256), 0, s, parent, N, stats);
}

void launch_cluster_queries(const half_t *rows, int row0, int n, int D, float *out, hipStream_t s) {
    const long pieces = (long)n * (D / 4);
    if (pieces > 0) hipLaunchKernelGGL(cluster_queries_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, s, rows, row0, n, D, out);
}

template <typename GT>
void launch_cluster_rerank_union(const GT *rows, int N, int D, const float *queries, int q_row0, int tile_origin, const ScreenScratch &w, float t,
                                 int32_t *parent, long long *stats, int *chunk_overflow, hipStream_t s) {
    hipLaunchKernelGGL((cluster_rerank_union_kernel<GT>), dim3(2048), dim3(128), (size_t)D * sizeof(float), s, rows, N, D, queries, q_row0, tile_origin,
                       reinterpret_cast<const MatchPair *>(w.pairs), w.pair_cap, w.ctl, t, parent, reinterpret_cast<unsigned long long *>(stats + 1),
                       chunk_overflow);
}
template void launch_cluster_rerank_union(const float *, int, int, const float *, int, int, const ScreenScratch &, float, int32_t *, long long *, int *, hipStream_t);
template void launch_cluster_rerank_union(const half_t *, int, int, const float *, int, int, const ScreenScratch &, float, int32_t *, long long *, int *, hipStream_t);

void launch_cluster_dense_union(const float *full, int F, int N, int q_row0, float t, int32_t *parent, long long *stats, hipStream_t s) {
    const long waves = (long)F * (((long)N + 63) / 64);
    const long blocks = (waves + 3) / 4;
    hipLaunchKernelGGL(cluster_dense_union_kernel, dim3((unsigned)(blocks < 4096 ? (blocks > 0 ? blocks : 1) : 4096)), dim3(256), 0, s, full, F, N, q_row0, t,
                       parent, reinterpret_cast<unsigned long long *>(stats + 1));
}

void launch_cluster_flatten(const int32_t *parent, int N, int32_t *labels, long long *stats, long long screened_chunks, long long dense_chunks,
                            hipStream_t s) {
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3((N + 255) / 256 > 0 ? (N + 255) / 256 : 1), dim3(256), 0, s, parent, N, labels, stats, screened_chunks,
                       dense_chunks);
}

// Triangle-mesh post-processing on the device (C ABI: include/ibgs_mesh.h; Python: ibgs_amd/mesh.py): the reference's post_process_mesh and
// clean_mesh (render.py:34-66), which call Open3D's cluster_connected_triangles / remove_triangles_by_mask / remove_unreferenced_vertices /
// remove_degenerate_triangles on the host.  This is the project's own statement of those routines ("Mesh post-processing");
// tests/mesh_ref.py restates it twice (scipy's connected_components, and a literal breadth-first search).
//
// CONTRACT
//   edges      triangle (a, b, c) has the three unordered index pairs {a,b}, {b,c}, {c,a}, taken literally ({a,a} is an edge like any other)
//   adjacency  two triangles are adjacent iff they have an edge in common (a shared vertex alone does not connect)
//   clusters   the connected components, numbered in ascending order of their smallest triangle index
//   filter     a triangle survives iff its cluster is kept; vertices no survivor refers to are dropped and the faces re-indexed; THEN survivors that
//              repeat a vertex index are dropped (so a vertex referenced only by a degenerate survivor stays); order is kept, rows are copied
//
// KERNELS (one thread per triangle unless said otherwise; ordering between the phases comes from kernel boundaries alone, nothing waits or spins)
//   mesh_init_kernel          parent[t] = t
//   mesh_edge_union_kernel    every edge goes into an open-addressing table keyed by the packed pair (lo << 32 | hi; 16-byte slots {key, triangle}, at least
//                             twice as many slots as edges, so it cannot fill).  The slot keeps the smallest triangle seen so far (atomicMin); an arrival that
//                             finds an earlier one there unites with it: an edge shared by n triangles costs n - 1 unions, whatever n.  No per-vertex
//                             lists: a fan apex of degree 10^5 is 10^5 different keys like any others.  (Edges bucketed by their lower vertex, matched
//                             inside the buckets, long buckets sent to this table, were measured and dropped: DESIGN.md section 11.)
//                             Union-find: always hook the LARGER root under the SMALLER (CAS on the root's parent word, relaxed, agent scope), path halving
//                             on the way up.  parent[x] <= x holds throughout, so the forest cannot close a cycle and a component's final root is its
//                             smallest triangle whatever the arrival order -- which is what the numbering rule needs and what makes the labels a pure
//                             function of the input.
//   mesh_flatten_kernel       parent[t] = root(t), flag[t] = (root == t)
//   (exclusive scan of the flags: scan_sort.hip)          cluster number of every root; the total is C
//   mesh_label_kernel         triangle_clusters, and counts / f64 areas by atomics: a wave walks 16 x 64 consecutive triangles and adds once per run of
//                             chunks that share a cluster
//   mesh_filter_mark_kernel   keep flag per triangle, referenced flag per vertex (plain stores of 1)
//   (two exclusive scans)     output position of every vertex and face; totals V', F'
//   mesh_emit_faces_kernel / mesh_emit_vertices_kernel (one thread per float)
// A face index outside [0, V) is never dereferenced: such triangles are counted in state[IBGS_MESH_BAD_FACES] and the caller fails the call.
#include "common.h"
#include "block_ops.h"
#include "../../include/ibgs_mesh.h"

namespace ibgs {

constexpr int MT = 256;          // threads per workgroup of every kernel here
constexpr unsigned long long MESH_EMPTY = ~0ull;
constexpr int MESH_MAX_ATTR = 8;

struct MeshSlot { unsigned long long key; uint32_t tri; uint32_t pad; };

struct MeshScratch {
    MeshSlot* slots; size_t nslots;          // a power of two >= 2 x 3 F
    uint32_t* parent;                        // F
    uint32_t* rootpos;                       // F + 1: root flags, then cluster number of every root; [F] = C
    uint32_t* vpos;                          // V + 1: referenced flags, then output row of every vertex; [V] = V'
    uint32_t* fpos;                          // F + 1: keep flags, then output row of every face; [F] = F'
    uint32_t* scan; size_t scan_elems;
    static MeshScratch carve(char* base, int64_t V, int64_t F, size_t* total)
    {
        MeshScratch m;
        Carver c(base);
        m.nslots = 64;
        while (m.nslots < (size_t)F * 6) m.nslots <<= 1;
        m.slots = c.take<MeshSlot>(m.nslots);
        m.parent = c.take<uint32_t>((size_t)F);
        m.rootpos = c.take<uint32_t>((size_t)F + 1);
        m.vpos = c.take<uint32_t>((size_t)V + 1);
        m.fpos = c.take<uint32_t>((size_t)F + 1);
        m.scan_elems = scan_scratch_elems((size_t)(V > F ? V : F) + 1);
        m.scan = c.take<uint32_t>(m.scan_elems);
        if (total) *total = c.cur - reinterpret_cast<uintptr_t>(base) + 128;
        return m;
    }
};

__device__ __forceinline__ uint32_t ld_agent(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ size_t mesh_hash(unsigned long long k)
{
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (size_t)k;
}

// root of x, halving the path on the way (every word written is an ancestor of its node: a racing reader only ever sees a shorter or an older path)
__device__ __forceinline__ uint32_t mesh_find(uint32_t* parent, uint32_t x)
{
    for (;;) {
        const uint32_t p = ld_agent(parent + x);
        if (p == x) return x;
        const uint32_t g = ld_agent(parent + p);
        if (g != p) st_agent(parent + x, g);
        x = g;
    }
}

// Hook the larger root under the smaller.  The CAS succeeds only on a word that still says "root"; a failed one hands back that node's new parent, from
// which the walk goes on: every retry starts strictly higher in the tree (lock-free, no waiting on any other thread).
__device__ __forceinline__ void mesh_unite(uint32_t* parent, uint32_t a, uint32_t b)
{
    for (;;) {
        a = mesh_find(parent, a);
        b = mesh_find(parent, b);
        if (a == b) return;
        if (a < b) { const uint32_t t = a; a = b; b = t; }
        const uint32_t old = atomicCAS(parent + a, a, b);
        if (old == a) return;
        a = old;
    }
}

// One edge into the table; the arrival unites with the smallest triangle the slot has seen.
__device__ __forceinline__ void mesh_edge_to_table(MeshSlot* slots, size_t mask, uint32_t p, uint32_t q, uint32_t t, uint32_t* parent, uint32_t* state)
{
    const unsigned long long key = ((unsigned long long)min(p, q) << 32) | max(p, q);
    size_t s = mesh_hash(key) & mask;
    for (size_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {
        unsigned long long cur = __hip_atomic_load(&slots[s].key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // half of the arrivals find their key
        if (cur == MESH_EMPTY) {
            cur = atomicCAS(&slots[s].key, MESH_EMPTY, key);
            if (cur == MESH_EMPTY) cur = key;
        }
        if (cur != key) continue;
        const uint32_t first = atomicMin(&slots[s].tri, t);          // 0xFFFFFFFF in an empty slot
        if (first != 0xFFFFFFFFu && first != t) mesh_unite(parent, t, first);
        return;
    }
    atomicAdd(state + IBGS_MESH_TABLE_FULL, 1u);
}

__global__ void __launch_bounds__(MT) mesh_init_kernel(uint32_t* __restrict__ parent, uint32_t F)
{
    const uint32_t t = blockIdx.x * MT + threadIdx.x;
    if (t < F) parent[t] = t;
}

__global__ void __launch_bounds__(MT) mesh_edge_union_kernel(const int32_t* __restrict__ faces, uint32_t V, uint32_t F, MeshSlot* slots, size_t mask,
                                                             uint32_t* parent, uint32_t* state)
{
    const uint32_t t = blockIdx.x * MT + threadIdx.x;
    if (t >= F) return;
    const uint32_t v[3] = {(uint32_t)faces[(size_t)t * 3], (uint32_t)faces[(size_t)t * 3 + 1], (uint32_t)faces[(size_t)t * 3 + 2]};
    if (v[0] >= V || v[1] >= V || v[2] >= V) { atomicAdd(state + IBGS_MESH_BAD_FACES, 1u); return; }          // (negative indices wrap above V)
    for (int e = 0; e < 3; ++e) mesh_edge_to_table(slots, mask, v[e], v[e == 2 ? 0 : e + 1], t, parent, state);
}

__global__ void __launch_bounds__(MT) mesh_flatten_kernel(uint32_t* parent, uint32_t* __restrict__ flag, uint32_t F)
{
    const uint32_t t = blockIdx.x * MT + threadIdx.x;
    if (t >= F) return;
    uint32_t x = t;
    for (uint32_t p; (p = ld_agent(parent + x)) != x;) x = p;
    st_agent(parent + t, x);          // (another thread walking through t sees its old parent or the root: both lead to the root)
    flag[t] = x == t ? 1u : 0u;
}

constexpr int LABEL_K = 16;          // chunks of 64 consecutive triangles per wave

// counts[lab] += n, areas[lab] += the wave's sum of a (one lane adds)
__device__ __forceinline__ void mesh_label_add(int32_t* counts, double* areas, uint32_t lab, int n, double a)
{
    a = wave_reduce(a, op_add());
    if ((threadIdx.x & 63) == 0 && n > 0) { atomicAdd(counts + lab, n); atomicAdd(areas + lab, a); }
}

// Marching cubes emits neighbouring triangles side by side, and one cluster usually holds most of the mesh: adding per triangle, or even per wave, queues
// up on that cluster's two words (measured: 11 ns per add on one address, 1.5 ms of a 4.1 M-face mesh).  A wave walks LABEL_K chunks of 64 consecutive
// triangles and keeps the running cluster's sums in registers for as long as whole chunks belong to it; a mixed chunk is added cluster by cluster.
__global__ void __launch_bounds__(MT) mesh_label_kernel(const float* __restrict__ vert, const int32_t* __restrict__ faces, uint32_t V, uint32_t F,
                                                        const uint32_t* __restrict__ parent, const uint32_t* __restrict__ rootpos,
                                                        int32_t* __restrict__ labels, int32_t* counts, double* areas, uint32_t* __restrict__ state)
{
    const int lane = threadIdx.x & 63;
    const size_t base = ((size_t)blockIdx.x * (MT / WAVE) + (threadIdx.x >> 6)) * (size_t)(WAVE * LABEL_K);
    if (blockIdx.x == 0 && threadIdx.x == 0) state[IBGS_MESH_CLUSTERS] = rootpos[F];
    uint32_t run = 0xFFFFFFFFu;          // the running cluster (wave-uniform), its triangles so far and this lane's share of their area
    int run_n = 0;
    double run_area = 0.0;
    for (int k = 0; k < LABEL_K; ++k) {
        const size_t t = base + (size_t)k * WAVE + lane;
        const bool valid = t < F;
        uint32_t lab = 0xFFFFFFFFu;
        double area = 0.0;
        if (valid) {
            lab = rootpos[parent[t]];
            labels[t] = (int32_t)lab;
            const uint32_t a = (uint32_t)faces[t * 3], b = (uint32_t)faces[t * 3 + 1], c = (uint32_t)faces[t * 3 + 2];
            if (a < V && b < V && c < V) {
                const double ax = vert[(size_t)a * 3], ay = vert[(size_t)a * 3 + 1], az = vert[(size_t)a * 3 + 2];
                const double ux = (double)vert[(size_t)b * 3] - ax, uy = (double)vert[(size_t)b * 3 + 1] - ay, uz = (double)vert[(size_t)b * 3 + 2] - az;
                const double wx = (double)vert[(size_t)c * 3] - ax, wy = (double)vert[(size_t)c * 3 + 1] - ay, wz = (double)vert[(size_t)c * 3 + 2] - az;
                const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
                area = 0.5 * sqrt(nx * nx + ny * ny + nz * nz);
            }
        }
        const unsigned long long live = __ballot(valid);
        if (live == 0ull) break;
        const uint32_t lead = (uint32_t)__shfl((int)lab, __ffsll((long long)live) - 1, WAVE);
        const bool uniform = __ballot(valid && lab != lead) == 0ull;
        if (uniform && lead == run) { run_n += (int)__popcll(live); run_area += area; continue; }
        mesh_label_add(counts, areas, run, run_n, run_area);
        if (uniform) { run = lead; run_n = (int)__popcll(live); run_area = area; continue; }
        run = 0xFFFFFFFFu; run_n = 0; run_area = 0.0;
        for (unsigned long long rem = live; rem != 0ull;) {
            const uint32_t cur = (uint32_t)__shfl((int)lab, __ffsll((long long)rem) - 1, WAVE);
            const unsigned long long same = __ballot(valid && lab == cur);
            mesh_label_add(counts, areas, cur, (int)__popcll(same), (valid && lab == cur) ? area : 0.0);
            rem &= ~same;
        }
    }
    mesh_label_add(counts, areas, run, run_n, run_area);
}

__global__ void __launch_bounds__(MT) mesh_filter_mark_kernel(const int32_t* __restrict__ faces, uint32_t V, uint32_t F, const int32_t* __restrict__ labels,
                                                              const uint8_t* __restrict__ keep_cluster, uint32_t C, uint32_t flags,
                                                              uint32_t* vflag, uint32_t* __restrict__ fflag, uint32_t* state)
{
    const uint32_t t = blockIdx.x * MT + threadIdx.x;
    if (t >= F) return;
    const uint32_t a = (uint32_t)faces[(size_t)t * 3], b = (uint32_t)faces[(size_t)t * 3 + 1], c = (uint32_t)faces[(size_t)t * 3 + 2];
    const uint32_t lab = (uint32_t)labels[t];
    bool keep = false;
    if (a >= V || b >= V || c >= V || lab >= C) atomicAdd(state + IBGS_MESH_BAD_FACES, 1u);
    else keep = keep_cluster[lab] != 0;
    if (keep && !(flags & IBGS_MESH_KEEP_VERTICES)) { vflag[a] = 1u; vflag[b] = 1u; vflag[c] = 1u; }
    if (keep && !(flags & IBGS_MESH_KEEP_DEGENERATE) && (a == b || b == c || c == a)) keep = false;
    fflag[t] = keep ? 1u : 0u;
}

__global__ void mesh_totals_kernel(const uint32_t* __restrict__ vpos, const uint32_t* __restrict__ fpos, uint32_t V, uint32_t F, uint32_t flags,
                                   uint32_t* __restrict__ state)
{
    state[IBGS_MESH_VERTICES_OUT] = (flags & IBGS_MESH_KEEP_VERTICES) ? V : vpos[V];
    state[IBGS_MESH_FACES_OUT] = fpos[F];
}

__global__ void __launch_bounds__(MT) mesh_emit_faces_kernel(const int32_t* __restrict__ faces, uint32_t V, uint32_t F, const uint32_t* __restrict__ vpos,
                                                             const uint32_t* __restrict__ fpos, uint32_t flags, uint32_t V_out, uint32_t F_out,
                                                             int32_t* __restrict__ faces_out, uint32_t* state)
{
    const uint32_t t = blockIdx.x * MT + threadIdx.x;
    if (t >= F) return;
    const uint32_t o = fpos[t];
    if (fpos[t + 1] == o) return;
    uint32_t v[3] = {(uint32_t)faces[(size_t)t * 3], (uint32_t)faces[(size_t)t * 3 + 1], (uint32_t)faces[(size_t)t * 3 + 2]};
    bool ok = o < F_out && v[0] < V && v[1] < V && v[2] < V;          // (a kept triangle's indices passed this test in the mark kernel already)
    if (ok && !(flags & IBGS_MESH_KEEP_VERTICES)) {
        for (int k = 0; k < 3; ++k) v[k] = vpos[v[k]];
        ok = v[0] < V_out && v[1] < V_out && v[2] < V_out;
    }
    if (!ok) { atomicAdd(state + IBGS_MESH_OVERRUN, 1u); return; }
    for (int k = 0; k < 3; ++k) faces_out[(size_t)o * 3 + k] = (int32_t)v[k];
}

struct MeshAttrs { const uint32_t* in[MESH_MAX_ATTR]; uint32_t* out[MESH_MAX_ATTR]; int n; };

// one thread per float of a vertex row: the reads are contiguous, the writes contiguous up to the gaps of the dropped rows
__global__ void __launch_bounds__(MT) mesh_emit_vertices_kernel(MeshAttrs at, uint32_t V, const uint32_t* __restrict__ vpos, uint32_t V_out, uint32_t* state)
{
    const size_t i = (size_t)blockIdx.x * MT + threadIdx.x;
    if (i >= (size_t)V * 3) return;
    const uint32_t v = (uint32_t)(i / 3), k = (uint32_t)(i - (size_t)v * 3);
    const uint32_t o = vpos[v];
    if (vpos[v + 1] == o) return;
    if (o >= V_out) { if (k == 0) atomicAdd(state + IBGS_MESH_OVERRUN, 1u); return; }
    for (int j = 0; j < at.n; ++j) at.out[j][(size_t)o * 3 + k] = at.in[j][i];          // words, not floats: bit for bit
}

static bool mesh_ok(const ibgs_mesh* m, const char* who, MeshScratch* sc)
{
    if (!m) { set_error("%s: null mesh", who); return false; }
    if (m->V < 0 || m->F < 0 || m->F >= (1 << 30)) { set_error("%s: V %d / F %d out of range (0 <= V < 2^31, 0 <= F < 2^30)", who, m->V, m->F); return false; }
    if ((m->V > 0 && !m->vertices) || (m->F > 0 && !m->faces) || !m->state || !m->scratch) { set_error("%s: null mesh array", who); return false; }
    size_t need = 0;
    *sc = MeshScratch::carve(static_cast<char*>(m->scratch), m->V, m->F, &need);
    return arena_ok(who, "scratch", m->scratch, m->scratch_bytes, need);
}

}  // namespace ibgs

using namespace ibgs;

extern "C" {

size_t ibgs_mesh_sizeof_mesh(void) { return sizeof(ibgs_mesh); }

size_t ibgs_mesh_required_scratch(int64_t V, int64_t F)
{
    if (V < 0 || F < 0 || V >= (int64_t(1) << 31) || F >= (int64_t(1) << 30)) return 0;
    size_t total = 0;
    MeshScratch::carve(nullptr, V, F, &total);
    return total;
}

int32_t ibgs_mesh_cluster(void* stream, const ibgs_mesh* mesh, int32_t* triangle_clusters, int32_t* cluster_n_triangles, double* cluster_area)
{
    MeshScratch sc;
    if (!mesh_ok(mesh, "mesh_cluster", &sc)) return -IBGS_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t V = (uint32_t)mesh->V, F = (uint32_t)mesh->F;
    if (F == 0) {
        IBGS_HIP(hipMemsetAsync(mesh->state + IBGS_MESH_CLUSTERS, 0, sizeof(uint32_t), s));
        return 0;
    }
    if (!triangle_clusters || !cluster_n_triangles || !cluster_area) { set_error("mesh_cluster: null output"); return -IBGS_ERR_INVALID; }
    IBGS_HIP(hipMemsetAsync(cluster_n_triangles, 0, (size_t)F * sizeof(int32_t), s));
    IBGS_HIP(hipMemsetAsync(cluster_area, 0, (size_t)F * sizeof(double), s));
    const unsigned g = grid_for(F, MT);
    IBGS_HIP(hipMemsetAsync(sc.slots, 0xFF, sc.nslots * sizeof(MeshSlot), s));
    hipLaunchKernelGGL(mesh_init_kernel, dim3(g), dim3(MT), 0, s, sc.parent, F);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(mesh_edge_union_kernel, dim3(g), dim3(MT), 0, s, mesh->faces, V, F, sc.slots, sc.nslots - 1, sc.parent, mesh->state);
    IBGS_HIP(hipGetLastError());
    hipLaunchKernelGGL(mesh_flatten_kernel, dim3(g), dim3(MT), 0, s, sc.parent, sc.rootpos, F);
    IBGS_HIP(hipGetLastError());
    int rc = exclusive_scan_u32(s, sc.rootpos, sc.rootpos, F, sc.scan, sc.scan_elems, true);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_label_kernel, dim3(grid_for(((size_t)F + LABEL_K - 1) / LABEL_K, MT)), dim3(MT), 0, s, mesh->vertices, mesh->faces, V, F, sc.parent, sc.rootpos, triangle_clusters,
                       cluster_n_triangles, cluster_area, mesh->state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_mesh_filter_count(void* stream, const ibgs_mesh* mesh, const int32_t* triangle_clusters, const uint8_t* keep_cluster, int32_t C, uint32_t flags)
{
    MeshScratch sc;
    if (!mesh_ok(mesh, "mesh_filter_count", &sc)) return -IBGS_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t V = (uint32_t)mesh->V, F = (uint32_t)mesh->F;
    if (C < 0 || (F > 0 && (!triangle_clusters || !keep_cluster))) { set_error("mesh_filter_count: bad C or null cluster arrays"); return -IBGS_ERR_INVALID; }
    if (!(flags & IBGS_MESH_KEEP_VERTICES)) IBGS_HIP(hipMemsetAsync(sc.vpos, 0, ((size_t)V + 1) * sizeof(uint32_t), s));
    IBGS_HIP(hipMemsetAsync(sc.fpos + F, 0, sizeof(uint32_t), s));
    if (F > 0) {
        hipLaunchKernelGGL(mesh_filter_mark_kernel, dim3(grid_for(F, MT)), dim3(MT), 0, s, mesh->faces, V, F, triangle_clusters, keep_cluster, (uint32_t)C, flags,
                           sc.vpos, sc.fpos, mesh->state);
        IBGS_HIP(hipGetLastError());
    }
    int rc = 0;
    if (!(flags & IBGS_MESH_KEEP_VERTICES)) rc = exclusive_scan_u32(s, sc.vpos, sc.vpos, V, sc.scan, sc.scan_elems, true);
    if (rc) return rc;
    rc = exclusive_scan_u32(s, sc.fpos, sc.fpos, F, sc.scan, sc.scan_elems, true);
    if (rc) return rc;
    hipLaunchKernelGGL(mesh_totals_kernel, dim3(1), dim3(1), 0, s, sc.vpos, sc.fpos, V, F, flags, mesh->state);
    IBGS_HIP(hipGetLastError());
    return 0;
}

int32_t ibgs_mesh_filter_emit(void* stream, const ibgs_mesh* mesh, uint32_t flags, int32_t V_out, int32_t F_out, int32_t* faces_out,
                              int32_t n_attr, const float* const* host_attr_in, float* const* host_attr_out)
{
    MeshScratch sc;
    if (!mesh_ok(mesh, "mesh_filter_emit", &sc)) return -IBGS_ERR_INVALID;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t V = (uint32_t)mesh->V, F = (uint32_t)mesh->F;
    const bool keep_v = (flags & IBGS_MESH_KEEP_VERTICES) != 0;
    if (V_out < 0 || F_out < 0 || V_out > mesh->V || F_out > mesh->F || (F_out > 0 && !faces_out) || n_attr < 0 || n_attr > MESH_MAX_ATTR
        || (keep_v && n_attr != 0) || (n_attr > 0 && (!host_attr_in || !host_attr_out))) {
        set_error("mesh_filter_emit: bad V' / F' / n_attr or null output"); return -IBGS_ERR_INVALID;
    }
    MeshAttrs at;
    at.n = n_attr;
    for (int j = 0; j < n_attr; ++j) {
        if (V > 0 && !host_attr_in[j]) { set_error("mesh_filter_emit: null attribute array %d", j); return -IBGS_ERR_INVALID; }
        if (V_out > 0 && !host_attr_out[j]) { set_error("mesh_filter_emit: null attribute output %d", j); return -IBGS_ERR_INVALID; }
        at.in[j] = reinterpret_cast<const uint32_t*>(host_attr_in[j]);
        at.out[j] = reinterpret_cast<uint32_t*>(host_attr_out[j]);
    }
    if (F > 0 && F_out > 0) {
        hipLaunchKernelGGL(mesh_emit_faces_kernel, dim3(grid_for(F, MT)), dim3(MT), 0, s, mesh->faces, V, F, sc.vpos, sc.fpos, flags, (uint32_t)V_out, (uint32_t)F_out,
                           faces_out, mesh->state);
        IBGS_HIP(hipGetLastError());
    }
    if (!keep_v && n_attr > 0 && V > 0 && V_out > 0) {
        hipLaunchKernelGGL(mesh_emit_vertices_kernel, dim3(grid_for((size_t)V * 3, MT)), dim3(MT), 0, s, at, V, sc.vpos, (uint32_t)V_out, mesh->state);
        IBGS_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"

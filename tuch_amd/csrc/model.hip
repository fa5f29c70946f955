// tuch_contact_model: uploads the per-model constants once (faces, bit-packed
// geodesic mask, segment tables, region tables).  The only place the library
// allocates device memory; the hot calls never do.  One builder per group of tables, called in the order of the uploads;
// what a later builder needs of an earlier one is an argument: the host tree (empty: the model has none), SegmentLists.
#include "model.h"
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include <unordered_map>

extern "C" int tuch_geomask_words(int V);

namespace {

// the segments as a CSR over their query vertices and faces (cap vertex c is index V + c), as the caller passes them
struct Segments {
    int count, num_caps;
    const int32_t *q_off, *q_vidx, *f_off, *faces;
};

// host forms of the segment tables that later builders read
struct SegmentLists {
    std::vector<int32_t> link_off{0}, links;       // seg_link_off, seg_link
    std::vector<int32_t> ray_off{0}, ray_ent;      // seg_ray_off, seg_ray_ent
    std::vector<int32_t> elem_mask;                // seg_elem_mask (empty without the leaf-assisted form)
};

// TUCH_DEBUG: why a model does without the leaf-assisted segment pass or the tree search
void debug_note(const char* fmt, ...)
{
    if (!getenv("TUCH_DEBUG")) return;
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
}

// bits[w][j], bit k = mask[perm[j]][perm[64 w + k]] for w < words (perm == nullptr: the identity)
std::vector<uint64_t> pack_mask(const uint8_t* mask, int V, int words, const int32_t* perm)
{
    std::vector<uint64_t> bits((size_t)words * V, 0);
    for (int j = 0; j < V; ++j) {
        const uint8_t* row = mask + (size_t)(perm ? perm[j] : j) * V;
        for (int i = 0; i < V; ++i)
            if (row[perm ? perm[i] : i]) bits[(size_t)(i >> 6) * V + j] |= (uint64_t)1 << (i & 63);
    }
    return bits;
}

bool mask_is_symmetric(const uint8_t* mask, int V)
{
    for (int a = 0; a < V; ++a)
        for (int b = a + 1; b < V; ++b)
            if ((mask[(size_t)a * V + b] != 0) != (mask[(size_t)b * V + a] != 0)) return false;
    return true;
}

void build_mesh_tables(tuch_contact_model* m, const int32_t* faces)
{
    const int32_t zero = 0;
    m->tables.put(&m->faces, faces, (size_t)m->F * 3);
    m->tables.put(&m->canary_hits, &zero, 1);
}

// The strip stream is what the flat form of the inside test walks: every model has one (tuch_build_strips opens a strip
// of at least three elements for every face not yet in one, so F >= 1 gives a non-empty stream).
int build_strip_tables(tuch_contact_model* m, const int32_t* faces)
{
    std::vector<int32_t> sv;
    std::vector<float> ss;
    tuch_build_strips(faces, m->F, sv, ss, &m->num_strips);
    TUCH_REQUIRE(!sv.empty(), "tuch_contact_model_create: no triangle strips for %d faces", m->F);
    m->strip_len = (int)sv.size();
    m->tables.put(&m->strip_vidx, sv.data(), sv.size());
    m->tables.put(&m->strip_sign, ss.data(), ss.size());
    return TUCH_OK;
}

// Face groups of the closest-point query: the faces ordered by their leaf (index order within a leaf; without a tree
// every face counts as leaf 0), cut wherever the leaf changes or a group has 64 faces; and the group of every face.
void build_closest_point_tables(tuch_contact_model* m)
{
    const int F = m->F, kGroup = 64;
    const std::vector<int32_t>& leaf = m->tree_face_leaf_host;
    std::vector<int32_t> list(F), off;
    for (int f = 0; f < F; ++f) list[f] = f;
    if (!leaf.empty()) std::stable_sort(list.begin(), list.end(), [&](int32_t a, int32_t b) { return leaf[a] < leaf[b]; });
    for (int i = 0; i < F; ++i)
        if (i == 0 || i - off.back() == kGroup || (!leaf.empty() && leaf[list[i]] != leaf[list[i - 1]])) off.push_back(i);
    m->cp_groups = (int)off.size();
    off.push_back(F);
    std::vector<int32_t> group(F);
    for (int g = 0; g + 1 < (int)off.size(); ++g)
        for (int i = off[g]; i < off[g + 1]; ++i) group[list[i]] = g;
    m->tables.put(&m->cp_face_list, list.data(), list.size());
    m->tables.put(&m->cp_group_off, off.data(), off.size());
    m->tables.put(&m->cp_face_group, group.data(), group.size());
}

// do the leaves' strip runs tile the exact part of the stream?  (ray_winding.hip poses the strip leaf by leaf)
bool leaf_runs_tile(const tuch_cluster_tree& t)
{
    std::vector<std::pair<int, int>> runs;
    for (int k = 0; k < t.num_leaves(); ++k)
        runs.emplace_back(t.node(t.leaf_node(k), kNodeExactOff), t.node(t.leaf_node(k), kNodeExactLen));
    std::sort(runs.begin(), runs.end());
    int at = 0;
    for (const auto& r : runs) { if (r.first != at) return false; at += r.second; }
    return at == t.exact_len;
}

// Cluster tree for the hierarchical winding numbers and its device copies; a mesh that is not a closed manifold (or has
// too many clusters for the LDS-resident boxes) simply keeps the flat strip path: the tree returned is empty then.
tuch_cluster_tree build_tree_tables(tuch_contact_model* m, const int32_t* faces)
{
    const int V = m->V, F = m->F;
    tuch_cluster_tree t;
    const char* e = getenv("TUCH_TREE_LEAF_FACES");
    // at most 1800 nodes: their slabs (80 B) and child indices (8 B) are staged in the CU's 160 KB of LDS by
    // tree_inner_bounds_kernel
    // 32 faces per leaf (SMPL: 430 leaves): measured best for the step at batch 64 -- 16: 104.5, 24: 109.2, 32: 110.3,
    // 40: 109.4, 48: 108.4, 64: 104.7, 96: 98.6 k body iterations/s (tighter slabs and boxes against more leaves to
    // test and emptier tiles); larger meshes get larger leaves so that the tree stays under the node limit below
    const int leaf_faces = e ? atoi(e) : (F / 850 > 32 ? F / 850 : 32);
    if (!tuch_cluster_tree_build_impl(V, F, faces, leaf_faces, t) || t.num_nodes > 1800) return tuch_cluster_tree();
    m->tree_nodes = t.num_nodes;
    m->tree_stream_len = t.stream_len;
    m->tree_exact_len = t.exact_len;
    m->tree_qblocks = t.num_qblocks;
    m->tree_heights = t.num_heights;
    m->tree_leaves = t.num_leaves();
    m->tree_leaf_runs_tile = leaf_runs_tile(t) ? 1 : 0;
    m->tree_num_frontiers = (int)t.frontier_off.size() - 1;
    m->tree_frontier_off_host = t.frontier_off;
    m->tree_face_leaf_host = t.face_leaf;
    m->tree_qperm_host = t.qperm;
    tuch_tables& tb = m->tables;
    tb.put(&m->tree_node, t.nodes.data(), t.nodes.size());
    tb.put(&m->tree_vidx, t.vidx.data(), t.vidx.size());
    tb.put(&m->tree_sign, t.sign.data(), t.sign.size());
    tb.put(&m->tree_qperm, t.qperm.data(), t.qperm.size());
    tb.put(&m->tree_height_off, t.height_off.data(), t.height_off.size());
    tb.put(&m->tree_height_nodes, t.height_nodes.data(), t.height_nodes.size());
    tb.put(&m->tree_frontier_nodes, t.frontier_nodes.data(), t.frontier_nodes.size());
    tb.put(&m->tree_launch_order, t.launch_order.data(), t.launch_order.size());
    tb.put(&m->tree_ancestors, t.ancestors.data(), t.ancestors.size());
    tb.put(&m->tree_rows, t.rows.data(), t.rows.size());
    // the search's leaf boxes carry a leaf's rows as first | count << 20 (v2v.hip)
    bool fits = V < (1 << 20);
    for (int k = 0; k < t.num_leaves(); ++k) fits = fits && t.leaf_rows(k).count < (1 << 11);
    m->tree_rows_pack = fits ? 1 : 0;
    return t;
}

// The mask in the tree's vertex order, and which (query block, node) pairs it rules out entirely; then the leaf tables
// of the search (model.h).
void build_tree_mask_tables(tuch_contact_model* m, const tuch_cluster_tree& t, const uint8_t* geomask)
{
    const int V = m->V, Wp = 2 * t.num_qblocks, N = t.num_nodes, L = t.num_leaves();
    tuch_tables& tb = m->tables;
    const std::vector<uint64_t> bits = pack_mask(geomask, V, Wp, t.qperm.data());
    // per 64-column block (one wavefront's columns) and node: the columns with ANY allowed row below the node
    std::vector<uint64_t> lanes((size_t)Wp * N, 0);
    for (int qb = 0; qb < Wp; ++qb) {
        const uint64_t* w0 = bits.data() + (size_t)qb * V;
        uint64_t* below = lanes.data() + (size_t)qb * N;
        for (int i = N - 1; i >= 0; --i) {
            if (!t.is_leaf(i)) { below[i] = below[t.child0(i)] | below[t.child1(i)]; continue; }
            const tuch_rows r = t.rows_of(i);
            for (int j = r.first; j < r.first + r.count; ++j) below[i] |= w0[j];
        }
    }
    tb.put(&m->tree_mask_bits, bits.data(), bits.size());
    tb.put(&m->tree_masked, lanes.data(), lanes.size());
    // The search's tables: leaves by their preorder sequence (= their position among the height-0 nodes); a subtree's
    // leaves are a contiguous range of it.  That needs height_nodes[0 .. L) in ascending node order, which the tree
    // builder gives by construction (cluster_tree.hip fills every height's nodes in one pass over i = 0 .. N).  A tree
    // that does not keep it gets none of the tables below, and a model without them has no tree search: the search runs
    // over all rows, as for a model without a tree (v2v.hip: use_v2v_tree).
    for (int k = 1; k < L; ++k)
        if (t.leaf_node(k) <= t.leaf_node(k - 1)) {
            debug_note("search: leaf %d out of node order, no tree search\n", k);
            return;
        }
    std::vector<int32_t> before(N + 1, 0), sub;            // before[i]: the leaves among the nodes ahead of node i
    for (int i = 0; i < N; ++i) before[i + 1] = before[i] + (t.is_leaf(i) ? 1 : 0);
    for (int lo : t.frontier_nodes) {
        sub.push_back(before[lo]);
        sub.push_back(before[t.skip(lo)] - before[lo]);
    }
    std::vector<uint64_t> by_leaf((size_t)Wp * L + 8, 0);        // + padding
    for (int qb = 0; qb < Wp; ++qb)
        for (int k = 0; k < L; ++k) by_leaf[(size_t)qb * L + k] = lanes[(size_t)qb * N + t.leaf_node(k)];
    tb.put(&m->tree_sub_leaf, sub.data(), sub.size());
    tb.put(&m->tree_masked_leaf, by_leaf.data(), by_leaf.size());
    // packed-row form: the leaves' rows in groups of four
    std::vector<int32_t> group(L + 1, 0);
    for (int k = 0; k < L; ++k) group[k + 1] = group[k] + (t.leaf_rows(k).count + 3) / 4;
    // for the leaf-major search (v2v.hip: the `pairs` condition of tuch_v2v_min_model): a leaf's rows fit one
    // 64-bit window of a column's mask row, and that row stands for the column's own admissible rows only if the mask is
    // symmetric
    for (int k = 0; k < L; ++k) m->tree_leaf_rows_max = std::max(m->tree_leaf_rows_max, t.leaf_rows(k).count);
    m->mask_symmetric = mask_is_symmetric(geomask, V) ? 1 : 0;
    const int G = group[L];
    std::vector<uint64_t> bits_g((size_t)Wp * G * 4 + 8, 0);
    for (int qb = 0; qb < Wp; ++qb)
        for (int k = 0; k < L; ++k) {
            const tuch_rows r = t.leaf_rows(k);
            for (int j = 0; j < r.count; ++j)
                bits_g[(size_t)qb * G * 4 + (size_t)group[k] * 4 + j] = bits[(size_t)qb * V + r.first + j];
        }
    m->tree_groups = G;
    tb.put(&m->tree_leaf_group, group.data(), group.size());
    tb.put(&m->tree_mask_bits_g, bits_g.data(), bits_g.size());
}

// Ordered one-rings (the tree exists, so the mesh is a closed manifold): face (v, a, b) in its cyclic order contributes
// the directed link edge a -> b; the link of v is the single cycle through them.  No tables when a link is not one cycle.
void build_ring_tables(tuch_contact_model* m, const int32_t* faces)
{
    const int V = m->V, F = m->F;
    std::vector<int32_t> deg(V + 1, 0);
    for (int i = 0; i < F * 3; ++i) ++deg[faces[i] + 1];
    for (int v = 0; v < V; ++v) deg[v + 1] += deg[v];
    std::vector<int32_t> from((size_t)F * 3), to((size_t)F * 3), fill(deg.begin(), deg.end() - 1);
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k) {
            const int v = faces[3 * f + k], slot = fill[v]++;
            from[slot] = faces[3 * f + (k + 1) % 3];
            to[slot] = faces[3 * f + (k + 2) % 3];
        }
    std::vector<int32_t> ring((size_t)F * 3);
    for (int v = 0; v < V; ++v) {
        const int lo = deg[v], n = deg[v + 1] - lo;
        if (n < 3) return;
        int cur = from[lo];
        for (int j = 0; j < n; ++j) {
            ring[lo + j] = cur;
            int nxt = -1;
            for (int e = lo; e < lo + n; ++e)
                if (from[e] == cur) { nxt = to[e]; break; }
            if (nxt < 0) return;
            cur = nxt;
        }
        if (cur != from[lo]) return;                    // the cycle must close after exactly n steps
        for (int j = 0; j < n; ++j)                     // ... and visit n distinct vertices
            for (int i = 0; i < j; ++i)
                if (ring[lo + i] == ring[lo + j]) return;
    }
    m->tables.put(&m->ring_off, deg.data(), deg.size());
    m->tables.put(&m->ring_vidx, ring.data(), ring.size());
}

// The segment tables as passed, their 64-query blocks and the caps.  A face index out of range fails the model.
void build_segment_tables(tuch_contact_model* m, const Segments& sg, const int32_t* cap_off, const int32_t* cap_vidx)
{
    m->num_segments = sg.count;
    m->num_caps = sg.num_caps;
    m->seg_q_total = sg.q_off[sg.count];
    m->seg_f_total = sg.f_off[sg.count];
    for (int i = 0; i < m->seg_f_total * 3; ++i)
        if (sg.faces[i] < 0 || sg.faces[i] >= m->V + sg.num_caps) {
            tuch_set_error("tuch_contact_model_create: segment face index %d out of range", sg.faces[i]);
            m->tables.rc = TUCH_ERR_ARG;
            return;
        }
    std::vector<int32_t> blocks, seg_of_q((size_t)m->seg_q_total);
    for (int s = 0; s < sg.count; ++s) {
        const int n = sg.q_off[s + 1] - sg.q_off[s];
        m->seg_q_max = std::max(m->seg_q_max, n);
        for (int q = 0; q < n; q += 64) { blocks.push_back(s); blocks.push_back(q); }
        for (int q = sg.q_off[s]; q < sg.q_off[s + 1]; ++q) seg_of_q[q] = s;
    }
    m->num_seg_blocks = (int)blocks.size() / 2;
    tuch_tables& tb = m->tables;
    tb.put(&m->seg_of_q, seg_of_q.data(), seg_of_q.size());
    tb.put(&m->seg_blocks, blocks.data(), blocks.size());
    tb.put(&m->seg_q_off, sg.q_off, (size_t)sg.count + 1);
    tb.put(&m->seg_q_vidx, sg.q_vidx, (size_t)m->seg_q_total);
    tb.put(&m->seg_f_off, sg.f_off, (size_t)sg.count + 1);
    tb.put(&m->seg_faces, sg.faces, (size_t)m->seg_f_total * 3);
    if (sg.num_caps > 0) {
        tb.put(&m->cap_off, cap_off, (size_t)sg.num_caps + 1);
        tb.put(&m->cap_vidx, cap_vidx, (size_t)cap_off[sg.num_caps]);
    }
}

// Tables for the ray-crossing form of the segment test: the star of every segment vertex as links, and the boundary
// chain of every segment mesh (model.h).
SegmentLists build_segment_ray_tables(tuch_contact_model* m, const Segments& sg)
{
    SegmentLists l;
    for (int s = 0; s < sg.count; ++s) {
        const int32_t* fs = sg.faces + 3 * (size_t)sg.f_off[s];
        const int nf = sg.f_off[s + 1] - sg.f_off[s];
        auto key = [](int a, int b) { return ((uint64_t)(uint32_t)a << 32) | (uint32_t)b; };
        std::unordered_map<uint64_t, int> net;                // directed edge -> occurrences - occurrences reversed
        std::unordered_map<int, std::vector<int32_t>> star;   // vertex -> (x, y) of its faces (v, x, y)
        for (int f = 0; f < nf; ++f)
            for (int k = 0; k < 3; ++k) {
                const int v = fs[3 * f + k], x = fs[3 * f + (k + 1) % 3], y = fs[3 * f + (k + 2) % 3];
                if (v < x) ++net[key(v, x)]; else --net[key(x, v)];
                star[v].push_back(x);
                star[v].push_back(y);
            }
        l.ray_ent.insert(l.ray_ent.end(), fs, fs + 3 * (size_t)nf);
        std::vector<uint64_t> open_edges;
        for (const auto& e : net)
            if (e.second != 0) open_edges.push_back(e.first);
        std::sort(open_edges.begin(), open_edges.end());      // a fixed order of the sums
        for (uint64_t e : open_edges) {
            const int a = (int)(e >> 32), b = (int)(uint32_t)e, mlt = net[e];
            // closing chain = links - boundary: the boundary edge x -> y enters with -multiplicity
            if (mlt > 0) l.ray_ent.insert(l.ray_ent.end(), {a, b, -mlt});
            else l.ray_ent.insert(l.ray_ent.end(), {b, a, mlt});
        }
        l.ray_off.push_back((int32_t)(l.ray_ent.size() / 3));
        for (int q = sg.q_off[s]; q < sg.q_off[s + 1]; ++q) {
            const auto it = star.find(sg.q_vidx[q]);
            if (it != star.end()) l.links.insert(l.links.end(), it->second.begin(), it->second.end());
            l.link_off.push_back((int32_t)(l.links.size() / 2));
        }
    }
    if (l.links.empty()) l.links.assign(2, 0);
    m->seg_ray_total = (int)(l.ray_ent.size() / 3);
    tuch_tables& tb = m->tables;
    tb.put(&m->seg_link_off, l.link_off.data(), l.link_off.size());
    tb.put(&m->seg_link, l.links.data(), l.links.size());
    tb.put(&m->seg_ray_off, l.ray_off.data(), l.ray_off.size());
    tb.put(&m->seg_ray_ent, l.ray_ent.data(), l.ray_ent.size());
    return l;
}

// a face by its rotation with the smallest id first: orientation kept
uint64_t face_key(int a, int b, int c)
{
    if (b < a && b < c) { const int t = a; a = b; b = c; c = t; }
    else if (c < a && c < b) { const int t = c; c = b; b = a; a = t; }
    return ((uint64_t)(uint32_t)a << 42) ^ ((uint64_t)(uint32_t)b << 21) ^ (uint64_t)(uint32_t)c;
}

// The caps a segment's entries (coff, cent) and links refer to: consecutive cap ids (the fused segment pass keeps a
// segment's centroids in LDS), segments in order; anything else (empty result) keeps the six-launch pass.
std::vector<int32_t> segment_cap_ranges(int V, const Segments& sg, const SegmentLists& l, const std::vector<int32_t>& coff,
                                        const std::vector<int32_t>& cent)
{
    std::vector<int32_t> crange(1, 0);
    for (int s = 0; s < sg.count; ++s) {
        int lo = sg.num_caps, hi = -1;
        auto see = [&](int id) { if (id >= V) { lo = std::min(lo, id - V); hi = std::max(hi, id - V); } };
        for (int e = coff[s]; e < coff[s + 1]; ++e)
            for (int k = 0; k < 3; ++k) see(cent[3 * (size_t)e + k]);
        for (int q = sg.q_off[s]; q < sg.q_off[s + 1]; ++q)
            for (int e = l.link_off[q]; e < l.link_off[q + 1]; ++e) { see(l.links[2 * (size_t)e]); see(l.links[2 * (size_t)e + 1]); }
        if (hi < 0) { crange.push_back(crange.back()); continue; }
        if (lo != crange.back() || hi - lo + 1 > 8) return {};
        crange.push_back(hi + 1);
    }
    return crange;
}

// Leaf-assisted form (model.h): which segments list every strip element's triangle, and the segments' entries without
// their body faces.  No tables unless every body face of a segment is a face of the model, listed once.
void build_leaf_assist_tables(tuch_contact_model* m, const tuch_cluster_tree& t, const int32_t* faces, const Segments& sg,
                              SegmentLists& l)
{
    const int V = m->V;
    // option seg_assist = 0: keep the segment pass self-contained (A/B, tests)
    if (t.num_nodes == 0 || t.exact_len == 0 || sg.count > 8 || m->opt.seg_assist == 0 || V >= (1 << 21)) return;
    std::unordered_map<uint64_t, int32_t> face_mask;      // body face -> segments that list it
    for (int f = 0; f < m->F; ++f) face_mask[face_key(faces[3 * f], faces[3 * f + 1], faces[3 * f + 2])] = 0;
    std::vector<int32_t> coff(1, 0), cent;
    for (int s = 0; s < sg.count; ++s) {
        for (int e = l.ray_off[s]; e < l.ray_off[s + 1]; ++e) {
            const int32_t* t3 = &l.ray_ent[3 * (size_t)e];
            if (!(t3[2] >= 0 && t3[0] < V && t3[1] < V && t3[2] < V)) {         // cap face or boundary edge
                cent.insert(cent.end(), t3, t3 + 3);
                continue;
            }
            const auto it = face_mask.find(face_key(t3[0], t3[1], t3[2]));       // a body face of the segment
            if (it == face_mask.end() || (it->second >> s) & 1) {
                debug_note("assist: seg %d face (%d %d %d) %s\n", s, t3[0], t3[1], t3[2],
                           it == face_mask.end() ? "not a body face" : "listed twice");
                return;
            }
            it->second |= 1 << s;
        }
        coff.push_back((int32_t)(cent.size() / 3));
    }
    std::vector<int32_t> vseg((size_t)V, 0);
    for (int s = 0; s < sg.count; ++s)
        for (int q = sg.q_off[s]; q < sg.q_off[s + 1]; ++q) vseg[sg.q_vidx[q]] |= 1 << s;
    std::vector<int32_t> emask((size_t)(t.exact_len + 2) / 3 * 3 + 6, 0),    // padded like the posed stream
                          vmask(t.qperm.size(), 0), vpos(V, 0);
    for (int p = 2; p < t.exact_len; ++p) {
        if (t.sign[p] == 0.0f) continue;
        int a = t.vidx[p - 2], b = t.vidx[p - 1];
        if (t.sign[p] < 0.0f) std::swap(a, b);                                // odd permutation of the face
        const auto it = face_mask.find(face_key(a, b, t.vidx[p]));
        if (it == face_mask.end()) { debug_note("assist: stream element %d not a face\n", p); return; }
        emask[p] = it->second;
    }
    for (size_t i = 0; i < t.qperm.size(); ++i) vmask[i] = vseg[t.qperm[i]];
    for (int i = V - 1; i >= 0; --i) vpos[t.qperm[i]] = i;
    if (cent.empty()) cent.assign(3, 0);
    m->seg_cap_total = coff.back();
    tuch_tables& tb = m->tables;
    tb.put(&m->seg_elem_mask, emask.data(), emask.size());
    tb.put(&m->seg_vmask, vmask.data(), vmask.size());
    tb.put(&m->seg_vpos, vpos.data(), vpos.size());
    tb.put(&m->seg_cap_off, coff.data(), coff.size());
    tb.put(&m->seg_cap_ent, cent.data(), cent.size());
    const std::vector<int32_t> crange = segment_cap_ranges(V, sg, l, coff, cent);
    tb.put(&m->seg_cap_range, crange.data(), crange.size());
    l.elem_mask = std::move(emask);
}

// Contact regions, and the geodesic mask restricted to every region pair (model.h)
void build_region_tables(tuch_contact_model* m, const uint8_t* geomask, int num_regions, const int32_t* region_off,
                         const int32_t* region_vidx, int num_pairs, const int32_t* pairs)
{
    m->num_regions = num_regions;
    m->num_pairs = num_pairs;
    auto size_of = [&](int r) { return region_off[r + 1] - region_off[r]; };
    for (int r = 0; r < num_regions; ++r) m->region_max = std::max(m->region_max, size_of(r));
    tuch_tables& tb = m->tables;
    tb.put(&m->region_off, region_off, (size_t)num_regions + 1);
    tb.put(&m->region_vidx, region_vidx, (size_t)region_off[num_regions]);
    if (num_pairs == 0) return;
    tb.put(&m->pairs, pairs, (size_t)num_pairs * 2);
    if (!geomask) return;
    std::vector<int64_t> off(num_pairs + 1, 0);
    for (int p = 0; p < num_pairs; ++p)
        off[p + 1] = off[p] + (int64_t)size_of(pairs[2 * p]) * ((size_of(pairs[2 * p + 1]) + 31) / 32);
    std::vector<uint32_t> words((size_t)off[num_pairs], 0u);
    for (int p = 0; p < num_pairs; ++p) {
        const int32_t* r1 = region_vidx + region_off[pairs[2 * p]];
        const int32_t* r2 = region_vidx + region_off[pairs[2 * p + 1]];
        const int n1 = size_of(pairs[2 * p]), n2 = size_of(pairs[2 * p + 1]), wpr = (n2 + 31) / 32;
        for (int a = 0; a < n1; ++a)
            for (int k = 0; k < n2; ++k)
                if (geomask[(size_t)r1[a] * m->V + r2[k]])
                    words[(size_t)off[p] + (size_t)a * wpr + (k >> 5)] |= 1u << (k & 31);
    }
    tb.put(&m->pair_mask, words.data(), words.size());
    tb.put(&m->pair_mask_off, off.data(), off.size());
}

// The fourth word of a posed strip element (ray_winding.hip: RayElem): the orientation as the INTEGER +1 / -1 / 0 in
// bits 0-23 and the element's segments (seg_elem_mask) in bits 24-31 -- both wave-uniform in the crossing kernel, read
// and tested on the scalar unit
void build_sign_words(tuch_contact_model* m, const tuch_cluster_tree& t, const std::vector<int32_t>& elem_mask)
{
    std::vector<int32_t> word(t.sign.size(), 0);
    for (size_t p = 0; p < word.size(); ++p) {
        const int32_t sg = t.sign[p] > 0.0f ? 1 : t.sign[p] < 0.0f ? -1 : 0;
        const int32_t em = p < elem_mask.size() ? elem_mask[p] : 0;
        word[p] = (int32_t)(((uint32_t)em << 24) | ((uint32_t)sg & 0xffffffu));
    }
    m->tables.put(&m->tree_sign_word, word.data(), word.size());
}

}  // namespace

extern "C" void tuch_contact_model_destroy(tuch_contact_model* m) { delete m; }

extern "C" int tuch_contact_model_create(
    tuch_contact_model** out, int V, int F, const int32_t* faces,
    const uint8_t* geomask,   // host [V,V] bytes (geod > geothres) or NULL
    int num_segments, const int32_t* seg_q_off, const int32_t* seg_q_vidx,
    const int32_t* seg_f_off, const int32_t* seg_faces,
    int num_caps, const int32_t* cap_off, const int32_t* cap_vidx,
    int num_regions, const int32_t* region_off, const int32_t* region_vidx,
    int num_pairs, const int32_t* pairs)
{
    TUCH_REQUIRE(out && faces && V > 0 && F > 0, "tuch_contact_model_create: bad mesh arguments");
    TUCH_REQUIRE(num_segments >= 0 && num_caps >= 0 && num_regions >= 0 && num_pairs >= 0,
                 "tuch_contact_model_create: negative table size");
    TUCH_REQUIRE(num_segments == 0 || (seg_q_off && seg_q_vidx && seg_f_off && seg_faces),
                 "tuch_contact_model_create: segment tables missing");
    TUCH_REQUIRE(num_caps == 0 || (cap_off && cap_vidx), "tuch_contact_model_create: cap tables missing");
    TUCH_REQUIRE(num_pairs == 0 || (num_regions > 0 && region_off && region_vidx && pairs),
                 "tuch_contact_model_create: region tables missing");
    for (int i = 0; i < F * 3; ++i)
        TUCH_REQUIRE(faces[i] >= 0 && faces[i] < V, "tuch_contact_model_create: face index %d out of range",
                     faces[i]);
    tuch_contact_model* m = new tuch_contact_model();   // every field zero, the options at their defaults
    m->V = V;
    m->F = F;
    tuch_options_from_env(&m->opt);          // the only place the hot calls' switches are read from the environment
    build_mesh_tables(m, faces);
    if (const int rc = build_strip_tables(m, faces)) {
        tuch_contact_model_destroy(m);
        return rc;
    }
    const tuch_cluster_tree tree = build_tree_tables(m, faces);
    if (tree.num_nodes > 0 && geomask) build_tree_mask_tables(m, tree, geomask);
    if (tree.num_nodes > 0) build_ring_tables(m, faces);
    build_closest_point_tables(m);
    if (geomask) {      // bits[w][j], bit k = geomask[j][64 w + k]
        const std::vector<uint64_t> bits = pack_mask(geomask, V, tuch_geomask_words(V), nullptr);
        m->tables.put(&m->mask_bits, bits.data(), bits.size());
    }
    SegmentLists lists;
    const Segments sg = {num_segments, num_caps, seg_q_off, seg_q_vidx, seg_f_off, seg_faces};
    if (num_segments > 0) build_segment_tables(m, sg, cap_off, cap_vidx);
    if (num_segments > 0 && m->tables.rc == TUCH_OK) {      // (the face indices are in range)
        lists = build_segment_ray_tables(m, sg);
        build_leaf_assist_tables(m, tree, faces, sg, lists);
    }
    if (num_regions > 0) build_region_tables(m, geomask, num_regions, region_off, region_vidx, num_pairs, pairs);
    if (!tree.sign.empty()) build_sign_words(m, tree, lists.elem_mask);
    const int rc = m->tables.rc;
    *out = rc == TUCH_OK ? m : nullptr;
    if (rc != TUCH_OK) tuch_contact_model_destroy(m);
    return rc;
}

namespace {
struct OptionName { const char* name; int tuch_options::*field; };
const OptionName kOptions[] = {
    {"winding_ray", &tuch_options::winding_ray}, {"winding_tree", &tuch_options::winding_tree},
    {"tree_waves", &tuch_options::tree_waves},
    {"ray_pair_cap", &tuch_options::ray_pair_cap}, {"ray_waves", &tuch_options::ray_waves},
    {"v2v_tree", &tuch_options::v2v_tree}, {"v2v_pairs", &tuch_options::v2v_pairs}, {"v2v_waves", &tuch_options::v2v_waves},
    {"seg_splits", &tuch_options::seg_splits}, {"seg_assist", &tuch_options::seg_assist}, {"seg_fused", &tuch_options::seg_fused},
    {"canary", &tuch_options::canary}, {"hd_search", &tuch_options::hd_search}, {"hd_search_waves", &tuch_options::hd_search_waves}, {"hd_overlap", &tuch_options::hd_overlap},
};
}  // namespace

void tuch_options_from_env(tuch_options* o)
{
    for (const OptionName& k : kOptions) {
        char env[64] = "TUCH_";
        size_t n = strlen(env);
        for (const char* c = k.name; *c && n + 1 < sizeof(env); ++c) env[n++] = (char)toupper((unsigned char)*c);
        env[n] = 0;
        const char* e = getenv(env);
        if (e && *e) o->*(k.field) = atoi(e);
    }
}

extern "C" int tuch_contact_model_set_option(tuch_contact_model* m, const char* name, int value)
{
    TUCH_REQUIRE(m && name, "tuch_contact_model_set_option: null argument");
    for (const OptionName& k : kOptions)
        if (!strcmp(k.name, name)) {
            TUCH_REQUIRE(strcmp(name, "seg_assist") != 0, "tuch_contact_model_set_option: seg_assist is fixed when the model "
                         "is created (TUCH_SEG_ASSIST)");
            m->opt.*(k.field) = value;
            return TUCH_OK;
        }
    tuch_set_error("tuch_contact_model_set_option: unknown option '%s'", name);
    return TUCH_ERR_ARG;
}

extern "C" int tuch_contact_model_canary_hits(const tuch_contact_model* m, int* hits_host, int reset)
{
    TUCH_REQUIRE(m && hits_host, "tuch_contact_model_canary_hits: null argument");
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(hits_host, m->canary_hits, sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        (reset && hipMemset(m->canary_hits, 0, sizeof(int32_t)) != hipSuccess)) {
        tuch_set_error("tuch_contact_model_canary_hits: %s", hipGetErrorString(hipGetLastError()));
        return TUCH_ERR_HIP;
    }
    return TUCH_OK;
}

extern "C" int tuch_contact_model_get_option(const tuch_contact_model* m, const char* name, int* value)
{
    TUCH_REQUIRE(m && name && value, "tuch_contact_model_get_option: null argument");
    if (!strcmp(name, "seg_fused_active")) {        // read-only: does the segment filter run as the one fused launch?
        *value = tuch_ray_segment_fused_available(m) ? 1 : 0;
        return TUCH_OK;
    }
    for (const OptionName& k : kOptions)
        if (!strcmp(k.name, name)) {
            *value = m->opt.*(k.field);
            return TUCH_OK;
        }
    tuch_set_error("tuch_contact_model_get_option: unknown option '%s'", name);
    return TUCH_ERR_ARG;
}

extern "C" const uint64_t* tuch_contact_model_mask_bits(const tuch_contact_model* m) { return m ? m->mask_bits : nullptr; }
extern "C" const uint64_t* tuch_contact_model_tree_mask_bits(const tuch_contact_model* m) { return m ? m->tree_mask_bits : nullptr; }

extern "C" int tuch_contact_model_tree_order(const tuch_contact_model* m, int32_t* qperm_host, int32_t* face_leaf_host)
{
    TUCH_REQUIRE(m, "tuch_contact_model_tree_order: null model");
    TUCH_REQUIRE(m->tree_nodes > 0, "tuch_contact_model_tree_order: the model has no cluster tree");
    if (qperm_host) memcpy(qperm_host, m->tree_qperm_host.data(), sizeof(int32_t) * m->V);
    if (face_leaf_host) memcpy(face_leaf_host, m->tree_face_leaf_host.data(), sizeof(int32_t) * m->F);
    return TUCH_OK;
}

extern "C" int tuch_contact_model_face_groups(const tuch_contact_model* m, int* num_groups, int32_t* group_off_host,
                                              int32_t* face_list_host, int32_t* face_group_host)
{
    TUCH_REQUIRE(m, "tuch_contact_model_face_groups: null model");
    TUCH_REQUIRE(m->cp_groups > 0 && m->cp_group_off && m->cp_face_list && m->cp_face_group,
                 "tuch_contact_model_face_groups: the model has no face groups");
    if (num_groups) *num_groups = m->cp_groups;
    if (group_off_host && tuch_table_download(group_off_host, m->cp_group_off, sizeof(int32_t) * (m->cp_groups + 1)) != TUCH_OK)
        return TUCH_ERR_HIP;
    if (face_list_host && tuch_table_download(face_list_host, m->cp_face_list, sizeof(int32_t) * m->F) != TUCH_OK)
        return TUCH_ERR_HIP;
    if (face_group_host && tuch_table_download(face_group_host, m->cp_face_group, sizeof(int32_t) * m->F) != TUCH_OK)
        return TUCH_ERR_HIP;
    return TUCH_OK;
}

extern "C" int tuch_contact_model_strips(const tuch_contact_model* m, int* stream_len, int* num_strips,
                                         int32_t* vidx_host, float* sign_host)
{
    TUCH_REQUIRE(m, "tuch_contact_model_strips: null model");
    if (stream_len) *stream_len = m->strip_len;
    if (num_strips) *num_strips = m->num_strips;
    if (vidx_host && tuch_table_download(vidx_host, m->strip_vidx, sizeof(int32_t) * m->strip_len) != TUCH_OK)
        return TUCH_ERR_HIP;
    if (sign_host && tuch_table_download(sign_host, m->strip_sign, sizeof(float) * m->strip_len) != TUCH_OK)
        return TUCH_ERR_HIP;
    return TUCH_OK;
}

extern "C" int tuch_contact_model_info(const tuch_contact_model* m, int* V, int* F, int* num_segments,
                                       int* seg_q_total, int* num_pairs)
{
    TUCH_REQUIRE(m, "tuch_contact_model_info: null model");
    if (V) *V = m->V;
    if (F) *F = m->F;
    if (num_segments) *num_segments = m->num_segments;
    if (seg_q_total) *seg_q_total = m->seg_q_total;
    if (num_pairs) *num_pairs = m->num_pairs;
    return TUCH_OK;
}

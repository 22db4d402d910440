// Test harness (CPU only, built by tests/test_scene_host.py with g++ -ffp-contract=off): the product's scene derivation
// (csrc/rt_scene_host.h build_host_scene) on real primitive lists.  Every scalar goes back to Python as a 32-bit word (floats
// as their bit patterns), named by scene_scalar_names() (":f" marks a float); every array as its bytes.
#include <cstdint>
#include <cstring>
#include <string>

#include "rt_scene_host.h"

namespace {

#define SHAPE_U32(X) X(n_sph) X(n_sph_pad) X(n_tri) X(bvh_depth) X(n_internal) X(root_ref) X(cull_pays) X(xcull_pays) X(quant_ok) \
    X(tri_ok) X(inverted_boxes) X(expanded)
#define SHAPE_F32(X) X(cull_density) X(r_slack) X(leaf_density)
#define SCENE_U32(X) X(n_big) X(has_order)
#define SCENE_F32(X) X(tri_k) X(tri_diag) X(tri_es) X(tri_e)
#define ARRAYS(X) X(geom, s->geom) X(geom_pk, s->geom_pk) X(geom_px, s->geom_px) X(mat, s->mat) X(emis, s->emis) X(tri, s->tri)     \
    X(tri_box, s->tri_box) X(geom_r, s->geom_r) X(big, s->big) X(world_rank, s->world_rank) X(nodes, s->bvh.nodes)                  \
    X(leaf_of, s->bvh.leaf_of) X(trav, s->bvh.trav) X(travq, s->bvh.travq)

uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

}  // namespace

extern "C" {

const char* scene_scalar_names() {
#define NAME_U(f) #f ","
#define NAME_F(f) #f ":f,"
    return SHAPE_U32(NAME_U) SHAPE_F32(NAME_F) SCENE_U32(NAME_U) SCENE_F32(NAME_F)
        "bvh_root_ref,bvh_depth_tree,grid_ok,grid_base0:f,grid_base1:f,grid_base2:f,grid_step0:f,grid_step1:f,grid_step2:f";
}

const char* scene_array_names() {
#define NAME_A(n, v) #n ","
    return ARRAYS(NAME_A);
}

void* scene_build(const rt_sphere* sp, uint32_t ns, const rt_triangle* tr, uint32_t nt, const uint32_t* world_index, int reorder) {
    rtscene::HostScene* s = new rtscene::HostScene;
    rtscene::build_host_scene(sp, ns, tr, nt, world_index, reorder != 0, *s);
    return s;
}

void scene_free(void* h) { delete (rtscene::HostScene*)h; }

void scene_scalars(const void* h, uint32_t* out) {
    const rtscene::HostScene* s = (const rtscene::HostScene*)h;
    int k = 0;
#define OUT_SU(f) out[k++] = (uint32_t)s->shape.f;
#define OUT_SF(f) out[k++] = bits(s->shape.f);
#define OUT_U(f) out[k++] = (uint32_t)s->f;
#define OUT_F(f) out[k++] = bits(s->f);
    SHAPE_U32(OUT_SU) SHAPE_F32(OUT_SF) SCENE_U32(OUT_U) SCENE_F32(OUT_F)
    out[k++] = s->bvh.root_ref;
    out[k++] = s->bvh.depth;
    out[k++] = s->bvh.grid.ok;
    for (int a = 0; a < 3; a++) out[k++] = bits(s->bvh.grid.base[a]);
    for (int a = 0; a < 3; a++) out[k++] = bits(s->bvh.grid.step[a]);
}

// the bytes of one array of the HostScene or its FlatBVH (nullptr: no such array)
const void* scene_array(const void* h, const char* name, uint64_t* bytes) {
    const rtscene::HostScene* s = (const rtscene::HostScene*)h;
    const std::string n = name;
#define ARRAY(nm, vec)                                \
    if (n == #nm) {                                   \
        *bytes = (vec).size() * sizeof((vec)[0]);     \
        return (vec).data();                          \
    }
    ARRAYS(ARRAY)
    return nullptr;
}

int scene_world_is_permutation(const uint32_t* world_index, uint32_t np) { return rtscene::world_is_permutation(world_index, np); }

// out: kk, dg, es, em of each of n triangles over its own box
void scene_tri_measures(const rt_triangle* t, uint32_t n, float* out) {
    for (uint32_t i = 0; i < n; i++) {
        const rtscene::TriMeasures m = rtscene::tri_measures(t[i], rtscene::tri_box(t[i]));
        out[4 * i] = m.kk;
        out[4 * i + 1] = m.dg;
        out[4 * i + 2] = m.es;
        out[4 * i + 3] = m.em;
    }
}

}  // extern "C"

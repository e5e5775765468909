/*
 * frag_host.cpp — the reference's fragment shader compiled as C++ and driven
 * over batches.  TEST INFRASTRUCTURE ONLY (oracle/Makefile, the `ref`
 * targets; bound by oracle/refpin.py).
 *
 * Everything in this file is this project's: a prelude standing in for the
 * shaders' shared header (the seven uniforms and the dimension constants), the
 * storage qualifiers defined away, and `main` renamed, because C++ keeps that
 * name.  The shader text itself is included by path from the reference tree
 * (-I$(REF)/src/shaders), unedited: render.frag in one namespace and, for
 * palette() and normal(), render.vert in a second one.
 *
 * Build (GCC only): -std=c++20 -O2 -fno-fast-math -ffp-contract=off
 * -fsingle-precision-constant.  The last flag makes a literal such as 0.3 a
 * float, as it is in GLSL; without it `0.3 * glow` is a double product.
 * Other dims by -DVXREF_X/Y/Z, powers of two only: Sf = 1 / dims must be exact.
 */
#include <cstring>

#include "glsl_shim.h"

#ifndef VXREF_X
#define VXREF_X 1024
#endif
#ifndef VXREF_Y
#define VXREF_Y 256
#endif
#ifndef VXREF_Z
#define VXREF_Z 32
#endif
static_assert((VXREF_X & (VXREF_X - 1)) == 0 && (VXREF_Y & (VXREF_Y - 1)) == 0 && (VXREF_Z & (VXREF_Z - 1)) == 0,
              "power-of-two dims only: Sf = 1 / dims must be exact");

/* the prelude both shaders share */
#define VXREF_PRELUDE                                      \
    using namespace glsl;                                  \
    int u_quality;                                         \
    mat4 u_matrix;                                         \
    ivec3 u_cellPos;                                       \
    vec3 u_fractPos;                                       \
    int u_frame;                                           \
    float u_time;                                          \
    vec3 u_sunDir;                                         \
    const int X = VXREF_X;                                 \
    const int Y = VXREF_Y;                                 \
    const int Z = VXREF_Z;                                 \
    const int c_glass = 7;                                 \
    const float Xf = float(X);                             \
    const float Yf = float(Y);                             \
    const float Zf = float(Z);                             \
    const vec3 Sf = 1.0f / vec3(Xf, Yf, Zf);               \
    vec4 gl_Position;

#define uniform
#define in
#define out
#define flat
#define smooth
#define highp
#define lowp
#define main vxref_shader_main

namespace vxfrag {
VXREF_PRELUDE
#include "render.frag"
}  // namespace vxfrag

namespace vxvert {
VXREF_PRELUDE
#include "render.vert"
}  // namespace vxvert

#undef uniform
#undef in
#undef out
#undef flat
#undef smooth
#undef highp
#undef lowp
#undef main

extern "C" {

/* X, Y, Z, c_glass, MAX_STEPS as ints; Xf, Yf, Zf, Sf.xyz as floats */
void vxref_constants(int ints[5], float floats[6]) {
    ints[0] = vxfrag::X; ints[1] = vxfrag::Y; ints[2] = vxfrag::Z; ints[3] = vxfrag::c_glass;
    ints[4] = vxfrag::MAX_STEPS;
    floats[0] = vxfrag::Xf; floats[1] = vxfrag::Yf; floats[2] = vxfrag::Zf;
    floats[3] = vxfrag::Sf.x; floats[4] = vxfrag::Sf.y; floats[5] = vxfrag::Sf.z;
}

/* field: X*Y*Z RGBA8 texels, x fastest; noise: w*h RGBA8, sides powers of two.  The caller keeps both alive. */
int vxref_bind(const uint8_t *field, int X, int Y, int Z, const uint8_t *noise, int w, int h) {
    if (X != vxfrag::X || Y != vxfrag::Y || Z != vxfrag::Z) return -1;
    if (w < 1 || h < 1 || (w & (w - 1)) || (h & (h - 1))) return -2;
    vxfrag::u_map.texels = field;
    vxfrag::u_map.w = X; vxfrag::u_map.h = Y; vxfrag::u_map.d = Z;
    vxfrag::u_noise.texels = noise;
    vxfrag::u_noise.w = w; vxfrag::u_noise.h = h;
    return 0;
}

void vxref_uniforms(int quality, const int cell[3], const float fract[3], float time, const float sun[3]) {
    vxfrag::u_quality = quality;
    vxfrag::u_cellPos = glsl::ivec3(cell[0], cell[1], cell[2]);
    vxfrag::u_fractPos = glsl::vec3(fract[0], fract[1], fract[2]);
    vxfrag::u_time = time;
    vxfrag::u_sunDir = glsl::vec3(sun[0], sun[1], sun[2]);
}

/* march() over n rays; every array holds 3 values per ray but min_dist and step */
void vxref_march(int n, const int *cell, const float *fract, const float *dir, int *o_cell, float *o_fract,
                 float *o_normal, float *o_min_dist, int *o_step) {
    for (int i = 0; i < n; i++) {
        const vxfrag::March m = vxfrag::march(glsl::ivec3(cell[3 * i], cell[3 * i + 1], cell[3 * i + 2]),
                                              glsl::vec3(fract[3 * i], fract[3 * i + 1], fract[3 * i + 2]),
                                              glsl::vec3(dir[3 * i], dir[3 * i + 1], dir[3 * i + 2]));
        o_cell[3 * i] = m.cellPos.x; o_cell[3 * i + 1] = m.cellPos.y; o_cell[3 * i + 2] = m.cellPos.z;
        o_fract[3 * i] = m.fractPos.x; o_fract[3 * i + 1] = m.fractPos.y; o_fract[3 * i + 2] = m.fractPos.z;
        o_normal[3 * i] = m.normal.x; o_normal[3 * i + 1] = m.normal.y; o_normal[3 * i + 2] = m.normal.z;
        o_min_dist[i] = m.minDist;
        o_step[i] = m.step;
    }
}

/* main() over n fragments: the varyings as the vertex shader forms them from a_color, a_normal and a_id */
void vxref_main(int n, const int *cell, const float *fract, const int *color, const int *normal, const int *id,
                float *o_color) {
    for (int i = 0; i < n; i++) {
        vxfrag::v_cellPos = glsl::ivec3(cell[3 * i], cell[3 * i + 1], cell[3 * i + 2]);
        vxfrag::v_fractPos = glsl::vec3(fract[3 * i], fract[3 * i + 1], fract[3 * i + 2]);
        vxfrag::v_color = vxvert::palette(color[i]);
        vxfrag::v_normal = vxvert::normal(normal[i]);
        vxfrag::v_id = id[i];
        vxfrag::vxref_shader_main();
        o_color[4 * i] = vxfrag::o_color.x; o_color[4 * i + 1] = vxfrag::o_color.y;
        o_color[4 * i + 2] = vxfrag::o_color.z; o_color[4 * i + 3] = vxfrag::o_color.w;
    }
}

void vxref_palette(int p, float rgb[3]) {
    const glsl::vec3 c = vxvert::palette(p);
    rgb[0] = c.x; rgb[1] = c.y; rgb[2] = c.z;
}

void vxref_normal(int n, float xyz[3]) {
    const glsl::vec3 c = vxvert::normal(n);
    xyz[0] = c.x; xyz[1] = c.y; xyz[2] = c.z;
}

}  // extern "C"

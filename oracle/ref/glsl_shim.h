/*
 * glsl_shim.h — the GLSL ES 3.00 subset the reference's two shaders use, as
 * C++ (g++), so that their text compiles unedited.  TEST INFRASTRUCTURE ONLY
 * (oracle/Makefile, the `ref` targets; see oracle/refpin.py).
 *
 * Every built-in is written from DESIGN.md §5 ("Numerical contract"), not from
 * the oracle: fp32, IEEE + - * / sqrt, no contraction (the recipe's flags),
 * min/max as selects, mix = x*(1-a) + y*a, dot left to right, one exp2
 * polynomial, ivec(float) with NaN -> 0 and saturation, unorm decode b/255,
 * texture at LOD 0 with fp32 weights and a nested lerp x -> y -> z.
 *
 * Swizzles are data members (unions over the components), so `v.rgb`, `v.xy`
 * read and, where the shaders assign them, write without parentheses.
 */
#ifndef VXREF_GLSL_SHIM_H
#define VXREF_GLSL_SHIM_H
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace glsl {

struct vec2;
struct vec3;
struct vec4;
struct ivec2;
struct ivec3;
struct bvec3;

/* ---- scalar built-ins ---- */
inline float min(float x, float y) { return y < x ? y : x; }
inline float max(float x, float y) { return x < y ? y : x; }
inline float clamp(float x, float a, float b) { return min(max(x, a), b); }
inline float floor(float x) { return std::floor(x); }               /* NaN -> NaN, +-0 -> +-0 */
inline float fract(float x) { return x - floor(x); }
inline float abs(float x) { return std::fabs(x); }                  /* clears the sign bit, of a NaN too */
inline float sign(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }   /* NaN, +-0 -> +0 */
inline float sqrt(float x) { return std::sqrt(x); }
inline float mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }
inline float sin(float x) { return std::sin(x); }                   /* rotate2d only: never called */
inline float cos(float x) { return std::cos(x); }

/* exp2: c_k = RN(ln2^k / k!), k = 9 .. 0 by Horner on f = x - floor(x), scaled by 2^floor(x) */
inline float exp2(float x) {
    if (x != x) return x;
    if (x >= 128.0f) return INFINITY;
    if (x < -126.0f) return 0.0f;
    const float n = floor(x);
    const float f = x - n;
    float p = 1.0178086e-07f;
    p = p * f + 1.3215487e-06f;
    p = p * f + 1.5252734e-05f;
    p = p * f + 1.5403530e-04f;
    p = p * f + 1.3333558e-03f;
    p = p * f + 9.6181291e-03f;
    p = p * f + 5.5504109e-02f;
    p = p * f + 2.4022651e-01f;
    p = p * f + 6.9314718e-01f;
    p = p * f + 1.0f;
    return std::ldexp(p, (int)n);
}
inline float exp(float x) { return exp2(x * 1.44269504f); }

/* int(float): NaN -> 0, saturating at +-2^24 */
inline int f2i(float x) {
    if (x != x) return 0;
    if (x > 16777216.0f) return 16777216;
    if (x < -16777216.0f) return -16777216;
    return (int)x;
}

/* ---- swizzle members: V = the vector type read, T = component, N = the host's size ---- */
template <class V, class T, int N, int A, int B>
struct swz2 {
    T v[N];
    operator V() const { return V(v[A], v[B]); }
};
template <class V, class T, int N, int A, int B, int C>
struct swz3 {
    T v[N];
    operator V() const { return V(v[A], v[B], v[C]); }
    swz3 &operator=(const V &o) {
        v[A] = o.x; v[B] = o.y; v[C] = o.z;
        return *this;
    }
    swz3 &operator*=(const V &o) {
        v[A] = v[A] * o.x; v[B] = v[B] * o.y; v[C] = v[C] * o.z;
        return *this;
    }
};

struct bvec3 {
    bool x, y, z;
    bvec3() : x(false), y(false), z(false) {}
    bvec3(bool a, bool b, bool c) : x(a), y(b), z(c) {}
};

struct ivec2 {
    int x, y;
    ivec2() : x(0), y(0) {}
    ivec2(int a, int b) : x(a), y(b) {}
};

struct ivec3 {
    union {
        struct { int x, y, z; };
        swz2<ivec2, int, 3, 0, 1> xy;
        swz3<ivec3, int, 3, 0, 1, 2> xyz;
    };
    ivec3() : x(0), y(0), z(0) {}
    ivec3(int a, int b, int c) : x(a), y(b), z(c) {}
    explicit ivec3(int a) : x(a), y(a), z(a) {}
    explicit ivec3(const vec3 &f);
    ivec3 &operator+=(const ivec3 &o) {
        x += o.x; y += o.y; z += o.z;
        return *this;
    }
};
inline ivec3 operator+(const ivec3 &a, const ivec3 &b) { return ivec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline ivec3 operator-(const ivec3 &a, const ivec3 &b) { return ivec3(a.x - b.x, a.y - b.y, a.z - b.z); }

struct vec2 {
    union {
        struct { float x, y; };
        struct { float r, g; };
    };
    vec2() : x(0.0f), y(0.0f) {}
    vec2(float a, float b) : x(a), y(b) {}
    explicit vec2(float a) : x(a), y(a) {}
    explicit vec2(const ivec2 &i) : x((float)i.x), y((float)i.y) {}
    vec2 &operator*=(float s) { x = x * s; y = y * s; return *this; }
    vec2 &operator*=(const vec2 &o) { x = x * o.x; y = y * o.y; return *this; }
    vec2 &operator+=(const vec2 &o) { x = x + o.x; y = y + o.y; return *this; }
};

struct vec3 {
    union {
        struct { float x, y, z; };
        struct { float r, g, b; };
        swz2<vec2, float, 3, 0, 1> xy;
        swz2<vec2, float, 3, 1, 2> yz;
        swz2<vec2, float, 3, 0, 1> rg;
        swz3<vec3, float, 3, 0, 1, 2> xyz;
        swz3<vec3, float, 3, 1, 2, 0> yzx;
        swz3<vec3, float, 3, 2, 0, 1> zxy;
        swz3<vec3, float, 3, 0, 1, 2> rgb;
    };
    vec3() : x(0.0f), y(0.0f), z(0.0f) {}
    vec3(float a, float b, float c) : x(a), y(b), z(c) {}
    explicit vec3(float a) : x(a), y(a), z(a) {}
    explicit vec3(const ivec3 &i) : x((float)i.x), y((float)i.y), z((float)i.z) {}
    explicit vec3(const bvec3 &b) : x(b.x ? 1.0f : 0.0f), y(b.y ? 1.0f : 0.0f), z(b.z ? 1.0f : 0.0f) {}
    vec3 &operator+=(const vec3 &o) { x = x + o.x; y = y + o.y; z = z + o.z; return *this; }
    vec3 &operator*=(const vec3 &o) { x = x * o.x; y = y * o.y; z = z * o.z; return *this; }
    vec3 &operator*=(float s) { x = x * s; y = y * s; z = z * s; return *this; }
    vec3 &operator/=(float s) { x = x / s; y = y / s; z = z / s; return *this; }
};

struct vec4 {
    union {
        struct { float x, y, z, w; };
        struct { float r, g, b, a; };
        swz3<vec3, float, 4, 0, 1, 2> rgb;
        swz3<vec3, float, 4, 0, 1, 2> xyz;
    };
    vec4() : x(0.0f), y(0.0f), z(0.0f), w(0.0f) {}
    vec4(float a, float b, float c, float d) : x(a), y(b), z(c), w(d) {}
    vec4(const vec3 &v, float d) : x(v.x), y(v.y), z(v.z), w(d) {}
    vec4(const ivec3 &v, float d) : x((float)v.x), y((float)v.y), z((float)v.z), w(d) {}
};

inline ivec3::ivec3(const vec3 &f) : x(f2i(f.x)), y(f2i(f.y)), z(f2i(f.z)) {}

/* column-major, as GLSL's constructors fill them */
struct mat3x3 {
    vec3 c0, c1, c2;
    mat3x3(float a0, float a1, float a2, float b0, float b1, float b2, float d0, float d1, float d2)
        : c0(a0, a1, a2), c1(b0, b1, b2), c2(d0, d1, d2) {}
};
struct mat4 {
    float m[16];
    mat4() : m{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1} {}
};

/* ---- arithmetic, component-wise; plain functions, so a swizzle member converts to its vector ---- */
inline vec2 operator+(const vec2 &a, const vec2 &b) { return vec2(a.x + b.x, a.y + b.y); }
inline vec2 operator-(const vec2 &a, const vec2 &b) { return vec2(a.x - b.x, a.y - b.y); }
inline vec2 operator*(const vec2 &a, const vec2 &b) { return vec2(a.x * b.x, a.y * b.y); }
inline vec2 operator+(const vec2 &a, float s) { return vec2(a.x + s, a.y + s); }
inline vec2 operator-(const vec2 &a, float s) { return vec2(a.x - s, a.y - s); }
inline vec2 operator*(const vec2 &a, float s) { return vec2(a.x * s, a.y * s); }
inline vec2 operator/(const vec2 &a, float s) { return vec2(a.x / s, a.y / s); }
inline vec2 operator+(float s, const vec2 &a) { return vec2(s + a.x, s + a.y); }
inline vec2 operator*(float s, const vec2 &a) { return vec2(s * a.x, s * a.y); }

inline vec3 operator-(const vec3 &a) { return vec3(-a.x, -a.y, -a.z); }
inline vec3 operator+(const vec3 &a, const vec3 &b) { return vec3(a.x + b.x, a.y + b.y, a.z + b.z); }
inline vec3 operator-(const vec3 &a, const vec3 &b) { return vec3(a.x - b.x, a.y - b.y, a.z - b.z); }
inline vec3 operator*(const vec3 &a, const vec3 &b) { return vec3(a.x * b.x, a.y * b.y, a.z * b.z); }
inline vec3 operator/(const vec3 &a, const vec3 &b) { return vec3(a.x / b.x, a.y / b.y, a.z / b.z); }
inline vec3 operator+(const vec3 &a, float s) { return vec3(a.x + s, a.y + s, a.z + s); }
inline vec3 operator*(const vec3 &a, float s) { return vec3(a.x * s, a.y * s, a.z * s); }
inline vec3 operator/(const vec3 &a, float s) { return vec3(a.x / s, a.y / s, a.z / s); }
inline vec3 operator*(float s, const vec3 &a) { return vec3(s * a.x, s * a.y, s * a.z); }
inline vec3 operator/(float s, const vec3 &a) { return vec3(s / a.x, s / a.y, s / a.z); }

inline vec4 operator*(float s, const vec4 &a) { return vec4(s * a.x, s * a.y, s * a.z, s * a.w); }
inline vec4 operator-(float s, const vec4 &a) { return vec4(s - a.x, s - a.y, s - a.z, s - a.w); }

/* M * v = c0 * v.x + c1 * v.y + c2 * v.z, summed left to right */
inline vec3 operator*(const mat3x3 &m, const vec3 &v) {
    return vec3((m.c0.x * v.x + m.c1.x * v.y) + m.c2.x * v.z, (m.c0.y * v.x + m.c1.y * v.y) + m.c2.y * v.z,
                (m.c0.z * v.x + m.c1.z * v.y) + m.c2.z * v.z);
}
inline vec4 operator*(const mat4 &m, const vec4 &v) {
    vec4 o;
    float *p[4] = {&o.x, &o.y, &o.z, &o.w};
    for (int i = 0; i < 4; i++) *p[i] = ((m.m[i] * v.x + m.m[4 + i] * v.y) + m.m[8 + i] * v.z) + m.m[12 + i] * v.w;
    return o;
}

/* ---- vector built-ins ---- */
inline vec3 floor(const vec3 &v) { return vec3(floor(v.x), floor(v.y), floor(v.z)); }
inline vec3 fract(const vec3 &v) { return vec3(fract(v.x), fract(v.y), fract(v.z)); }
inline vec3 abs(const vec3 &v) { return vec3(abs(v.x), abs(v.y), abs(v.z)); }
inline vec3 sign(const vec3 &v) { return vec3(sign(v.x), sign(v.y), sign(v.z)); }
inline vec3 min(const vec3 &a, const vec3 &b) { return vec3(min(a.x, b.x), min(a.y, b.y), min(a.z, b.z)); }
inline vec3 max(const vec3 &a, const vec3 &b) { return vec3(max(a.x, b.x), max(a.y, b.y), max(a.z, b.z)); }
inline vec3 clamp(const vec3 &v, const vec3 &a, const vec3 &b) { return min(max(v, a), b); }
inline vec3 mix(const vec3 &x, const vec3 &y, float a) { return vec3(mix(x.x, y.x, a), mix(x.y, y.y, a), mix(x.z, y.z, a)); }
inline float dot(const vec2 &a, const vec2 &b) { return a.x * b.x + a.y * b.y; }
inline float dot(const vec3 &a, const vec3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline float length(const vec2 &v) { return sqrt(dot(v, v)); }
inline float length(const vec3 &v) { return sqrt(dot(v, v)); }
inline vec3 normalize(const vec3 &v) { return v / sqrt(dot(v, v)); }
inline vec3 reflect(const vec3 &I, const vec3 &N) { return I - (2.0f * dot(N, I)) * N; }

/* comparisons: false on a NaN operand, as IEEE's */
inline bvec3 lessThanEqual(const vec3 &a, const vec3 &b) { return bvec3(a.x <= b.x, a.y <= b.y, a.z <= b.z); }
inline bvec3 lessThan(const ivec3 &a, const ivec3 &b) { return bvec3(a.x < b.x, a.y < b.y, a.z < b.z); }
inline bvec3 greaterThanEqual(const ivec3 &a, const ivec3 &b) { return bvec3(a.x >= b.x, a.y >= b.y, a.z >= b.z); }
inline bool any(const bvec3 &b) { return b.x || b.y || b.z; }

/* ---- samplers: RGBA8 texels, x fastest; unorm decode b / 255 ---- */
struct sampler2D {
    const uint8_t *texels = nullptr;
    int w = 0, h = 0;                  /* powers of two (REPEAT) */
};
struct sampler3D {
    const uint8_t *texels = nullptr;
    int w = 0, h = 0, d = 0;
};
inline float unorm(uint8_t b) { return (float)b / 255.0f; }
inline vec4 texel4(const uint8_t *t) { return vec4(unorm(t[0]), unorm(t[1]), unorm(t[2]), unorm(t[3])); }
inline vec4 lerp4(const vec4 &p, const vec4 &q, float a) {
    return vec4(mix(p.x, q.x, a), mix(p.y, q.y, a), mix(p.z, q.z, a), mix(p.w, q.w, a));
}

inline vec4 texelFetch(const sampler3D &s, const ivec3 &c, int /*lod*/) {
    return texel4(s.texels + 4 * ((size_t)c.x + (size_t)s.w * ((size_t)c.y + (size_t)s.h * (size_t)c.z)));
}

/* one axis of a LINEAR lookup: u = coord * size - 0.5, texels floor(u) and floor(u) + 1, weight fract(u) */
inline void axis_clamp(float coord, int size, int &i0, int &i1, float &a) {
    const float u = coord * (float)size - 0.5f;
    const float fl = floor(u);
    a = u - fl;
    const int i = f2i(fl), j = i + 1;
    i0 = i < 0 ? 0 : (i > size - 1 ? size - 1 : i);          /* CLAMP_TO_EDGE */
    i1 = j < 0 ? 0 : (j > size - 1 ? size - 1 : j);
}
inline void axis_repeat(float coord, int size, int &i0, int &i1, float &a) {
    const float u = coord * (float)size - 0.5f;
    const float fl = floor(u);
    a = u - fl;
    const float q = floor(fl / (float)size);                 /* REPEAT: fl mod size, size a power of two */
    i0 = f2i(fl - q * (float)size) & (size - 1);
    i1 = (i0 + 1) & (size - 1);
}

inline vec4 texture(const sampler3D &s, const vec3 &p) {
    int x0, x1, y0, y1, z0, z1;
    float ax, ay, az;
    axis_clamp(p.x, s.w, x0, x1, ax);
    axis_clamp(p.y, s.h, y0, y1, ay);
    axis_clamp(p.z, s.d, z0, z1, az);
    auto at = [&](int x, int y, int z) {
        return texel4(s.texels + 4 * ((size_t)x + (size_t)s.w * ((size_t)y + (size_t)s.h * (size_t)z)));
    };
    const vec4 r00 = lerp4(at(x0, y0, z0), at(x1, y0, z0), ax), r10 = lerp4(at(x0, y1, z0), at(x1, y1, z0), ax);
    const vec4 r01 = lerp4(at(x0, y0, z1), at(x1, y0, z1), ax), r11 = lerp4(at(x0, y1, z1), at(x1, y1, z1), ax);
    return lerp4(lerp4(r00, r10, ay), lerp4(r01, r11, ay), az);
}

inline vec4 texture(const sampler2D &s, const vec2 &p) {
    int x0, x1, y0, y1;
    float ax, ay;
    axis_repeat(p.x, s.w, x0, x1, ax);
    axis_repeat(p.y, s.h, y0, y1, ay);
    auto at = [&](int x, int y) { return texel4(s.texels + 4 * ((size_t)y * (size_t)s.w + (size_t)x)); };
    return lerp4(lerp4(at(x0, y0), at(x1, y0), ax), lerp4(at(x0, y1), at(x1, y1), ax), ay);
}

}  // namespace glsl
#endif

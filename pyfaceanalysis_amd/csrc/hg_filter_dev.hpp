// Device helpers shared by the files that restate PIL's BILINEAR / BICUBIC transform (hg_extract.hip: windows; hg_normalize.hip:
// pose-normalised faces): the no-contraction double operators, the coordinate entry of PIL's affine_transform and the two filters of
// Geometry.c.  Include it inside the including file's anonymous namespace, after <hip/hip_runtime.h> and include/higsfa.h.
//
// No contraction anywhere below: under hipcc's -ffp-contract=fast-honor-pragmas the __dadd_rn / __dmul_rn of the HIP headers are plain
// operators, so a multiply feeding an add may become one fma.  The helpers are defined under the pragma: each operation rounds on its
// own, as PIL's C doubles and Python floats do (tests/test_fp_contract.py checks the fma count).
#pragma once
#pragma clang fp contract(off)

__device__ __forceinline__ double d_add(double a, double b) { return a + b; }
__device__ __forceinline__ double d_sub(double a, double b) { return a - b; }
__device__ __forceinline__ double d_mul(double a, double b) { return a * b; }
__device__ __forceinline__ double d_div(double a, double b) { return a / b; }

// PIL's ImagingGenericTransform with affine_transform and bilinear_filter8 / bicubic_filter8 (Geometry.c), for uint8 frames.  An
// EXTENT window is separable: the source coordinate of output column ox depends on ox alone, so a box has a table of w + h
// entries as for NEAREST, each holding the integer part and the fraction of its coordinate (`i` = kFiltOutside where PIL's range test
// leaves the output pixel 0).  Unlike the NEAREST tables these are closed forms, one multiply-add per entry: PIL evaluates the affine
// map per pixel, it has no running sum here.
struct FiltEnt {
    double d;       // fraction: (xs - 0.5) - floor(xs - 0.5)
    int32_t i;      // floor(xs - 0.5), in [-1, size - 1]
    int32_t pad;
};
constexpr int32_t kFiltOutside = INT32_MIN;

__device__ __forceinline__ FiltEnt filter_coord(double s, int lim) {
    FiltEnt e;
    e.pad = 0;
    if (!(s >= 0.0 && s < (double)lim)) {       // (a NaN coordinate is outside too: nothing below may turn it into an index)
        e.i = kFiltOutside;
        e.d = 0.0;
        return e;
    }
    s = d_sub(s, 0.5);
    e.i = s < 0.0 ? (int)floor(s) : (int)s;      // Geometry.c FLOOR()
    e.d = d_sub(s, (double)e.i);
    return e;
}

__device__ __forceinline__ double bicubic(double v1, double v2, double v3, double v4, double d) {      // Geometry.c BICUBIC(), a = -0.5
    const double p1 = v2;
    const double p2 = d_add(-v1, v3);
    const double p3 = d_sub(d_add(d_mul(2.0, d_sub(v1, v2)), v3), v4);
    const double p4 = d_add(d_sub(d_add(-v1, v2), v3), v4);
    return d_add(p1, d_mul(d, d_add(p2, d_mul(d, d_add(p3, d_mul(d, p4))))));
}

// One filtered, quantised pixel at (x + dx, y + dy) of a W x H uint8 image whose pixels come from tap(column, row); every
// coordinate handed to tap lies inside the image.
template <int F, typename Tap>
__device__ __forceinline__ uint8_t filter_sample(Tap&& tap, int x, double dx, int y, double dy, int W, int H) {
    auto clipx = [&](int v) { return v < 0 ? 0 : v < W ? v : W - 1; };
    if constexpr (F == HG_FILTER_BILINEAR) {
        const int x0 = clipx(x), x1 = clipx(x + 1);
        auto row = [&](int yy) {
            const double p0 = tap(x0, yy), p1 = tap(x1, yy);
            return d_add(p0, d_mul(d_sub(p1, p0), dx));
        };
        const double v1 = row(y < 0 ? 0 : y);
        const double v2 = y + 1 < H ? row(y + 1) : v1;
        return (uint8_t)(int)d_add(v1, d_mul(d_sub(v2, v1), dy));
    } else {
        const int x0 = clipx(x - 1), x1 = clipx(x), x2 = clipx(x + 1), x3 = clipx(x + 2);
        auto row = [&](int yy) { return bicubic(tap(x0, yy), tap(x1, yy), tap(x2, yy), tap(x3, yy), dx); };
        const double r1 = row(y - 1 < 0 ? 0 : y - 1);
        const double r2 = y >= 0 ? row(y) : r1;          // (y <= H - 1 always)
        const double r3 = y + 1 < H ? row(y + 1) : r2;
        const double r4 = y + 2 < H ? row(y + 2) : r3;
        const double v = bicubic(r1, r2, r3, r4, dy);
        return v <= 0.0 ? (uint8_t)0 : v >= 255.0 ? (uint8_t)255 : (uint8_t)(int)v;
    }
}

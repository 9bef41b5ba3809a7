// cam_model.h - lens distortion models: the forward map normalised -> raw pixel, its inverse by Newton's method
// with a per-point status, and one entry of the fixed-point rectification map.  The same text runs in the kernels of camera.hip
// and on the host (tests/camera_twin.cpp builds it with a plain C++ compiler): f64, contraction off, the operations in the
// order written.  Only + - * / and sqrt (correctly rounded on both builds) are used - the atan and tan of the equidistant model
// are cam_atan and cam_tan below, series in the four operations - so both builds give the same bits for every model.
#pragma once
#pragma clang fp contract(off)
#include <stdint.h>
#include <math.h>

#ifdef __HIPCC__
#define CAM_HD __host__ __device__ __forceinline__
#else
#define CAM_HD inline
#endif

#define CAM_RECORD 16           // doubles per camera record (SLAM_CAM_RECORD)
#define CAM_PINHOLE 0
#define CAM_RADTAN 1            // k = (k1, k2, p1, p2, k3)
#define CAM_EQUIDISTANT 2       // k = (k1, k2, k3, k4)
#define CAM_OK 0
#define CAM_NOT_CONVERGED 1
#define CAM_NO_IMAGE 2
#define CAM_NOT_FINITE 3
#define CAM_THETA_MAX 1.5       // equidistant: an angle of 1.5 rad or more from the axis has no pinhole image worth the name
#define CAM_MAP_SENTINEL INT32_MIN
#define CAM_DBL_MAX 1.7976931348623157e308

// the record of include/slamhip.h: f64 [16] = {fx, fy, cx, cy, model, k[0..7], 0, 0, 0}
struct cam_rec {
    double fx, fy, cx, cy, model;
    double k[8];
    double pad[3];
};

struct cam_point {
    double x, y;        // normalised coordinates (undistort) / distorted normalised coordinates (distort)
    double u, v;        // pixel
    int status;
};

CAM_HD bool cam_finite(double a) { return fabs(a) <= CAM_DBL_MAX; }
CAM_HD double cam_max(double a, double b) { return a > b ? a : b; }

// ---- forward: normalised (x, y) -> distorted normalised (xd, yd) ---------------------------------------------------------
CAM_HD void cam_radtan_n(const double* k, double x, double y, double* xd, double* yd) {
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
    const double r2 = x * x + y * y;
    const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
    *xd = (x * rad + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x);
    *yd = (y * rad + p1 * (r2 + (2.0 * y) * y)) + ((2.0 * p2) * x) * y;
}

// ---- atan and tan in + - * / only -------------------------------------------------------------------------------------------
// The equidistant model needs atan (forward) and tan (inverse).  The math libraries of the two builds differ by a few ulp there,
// which would be the only difference between them; these two give the same bits on both, within about 2 ulp of the true value.
#define CAM_PIO2_HI 1.5707963267948966
#define CAM_PIO2_LO 6.123233995736766e-17

// atan(r), r >= 0 (inf gives pi/2, NaN gives NaN).  r > 1: pi/2 - atan(1 / r).  r <= 1: with c the nearest of 0, 1/4, 1/2, 3/4, 1
// atan(r) = atan(c) + atan(t), t = (r - c) / (1 + r c), |t| <= 1/8, atan(t) = t - t z (1/3 - z (1/5 - ... z / 25)), z = t t.
CAM_HD double cam_atan(double r) {
    const bool flip = r > 1.0;
    const double q = flip ? 1.0 / r : r;
    const int k = q <= 1.0 ? (int)(4.0 * q + 0.5) : 0;            // (a NaN takes c = 0 and comes out as a NaN)
    const double c = 0.25 * (double)k;
    const double hi = k == 0 ? 0.0 : k == 1 ? 0.24497866312686414 : k == 2 ? 0.4636476090008061 : k == 3 ? 0.6435011087932844 : 0.7853981633974483;
    const double lo = k == 0 ? 0.0 : k == 1 ? 1.0698755618734451e-17 : k == 2 ? 2.2698777452961687e-17 : k == 3 ? 1.5834785051444286e-17 : 3.061616997868383e-17;
    const double t = (q - c) / (1.0 + q * c);
    const double z = t * t;
    double p = 1.0 / 25.0;
    p = 1.0 / 23.0 - z * p;
    p = 1.0 / 21.0 - z * p;
    p = 1.0 / 19.0 - z * p;
    p = 1.0 / 17.0 - z * p;
    p = 1.0 / 15.0 - z * p;
    p = 1.0 / 13.0 - z * p;
    p = 1.0 / 11.0 - z * p;
    p = 1.0 / 9.0 - z * p;
    p = 1.0 / 7.0 - z * p;
    p = 1.0 / 5.0 - z * p;
    p = 1.0 / 3.0 - z * p;
    const double a = hi + ((t - (t * z) * p) + lo);
    return flip ? (CAM_PIO2_HI - a) + CAM_PIO2_LO : a;
}

// tan(t), 0 <= t < pi/2 (used below 1.5).  t <= pi/4: sin(t) / cos(t); else with y = pi/2 - t: cos(y) / sin(y); both by their
// Taylor series to y^27 / y^26 on |y| <= pi/4 (the first term left out is below 1e-30).
CAM_HD double cam_tan(double t) {
    const bool flip = t > 0.7853981633974483;
    const double y = flip ? (CAM_PIO2_HI - t) + CAM_PIO2_LO : t;
    const double z = y * y;
    double s = 1.0 / 10888869450418352160768000000.0;             // 1 / 27!
    s = 1.0 / 15511210043330985984000000.0 - z * s;               // 1 / 25!
    s = 1.0 / 25852016738884976640000.0 - z * s;                  // 1 / 23!
    s = 1.0 / 51090942171709440000.0 - z * s;                     // 1 / 21!
    s = 1.0 / 121645100408832000.0 - z * s;                       // 1 / 19!
    s = 1.0 / 355687428096000.0 - z * s;                          // 1 / 17!
    s = 1.0 / 1307674368000.0 - z * s;                            // 1 / 15!
    s = 1.0 / 6227020800.0 - z * s;                               // 1 / 13!
    s = 1.0 / 39916800.0 - z * s;                                 // 1 / 11!
    s = 1.0 / 362880.0 - z * s;                                   // 1 / 9!
    s = 1.0 / 5040.0 - z * s;                                     // 1 / 7!
    s = 1.0 / 120.0 - z * s;                                      // 1 / 5!
    s = 1.0 / 6.0 - z * s;                                        // 1 / 3!
    const double sn = y - (y * z) * s;
    double c = 1.0 / 403291461126605635584000000.0;               // 1 / 26!
    c = 1.0 / 620448401733239439360000.0 - z * c;                 // 1 / 24!
    c = 1.0 / 1124000727777607680000.0 - z * c;                   // 1 / 22!
    c = 1.0 / 2432902008176640000.0 - z * c;                      // 1 / 20!
    c = 1.0 / 6402373705728000.0 - z * c;                         // 1 / 18!
    c = 1.0 / 20922789888000.0 - z * c;                           // 1 / 16!
    c = 1.0 / 87178291200.0 - z * c;                              // 1 / 14!
    c = 1.0 / 479001600.0 - z * c;                                // 1 / 12!
    c = 1.0 / 3628800.0 - z * c;                                  // 1 / 10!
    c = 1.0 / 40320.0 - z * c;                                    // 1 / 8!
    c = 1.0 / 720.0 - z * c;                                      // 1 / 6!
    c = 1.0 / 24.0 - z * c;                                       // 1 / 4!
    const double cs = (1.0 - 0.5 * z) + (z * z) * c;
    return flip ? cs / sn : sn / cs;
}

// theta_d of the equidistant model
CAM_HD double cam_equi_poly(const double* k, double t) {
    const double t2 = t * t;
    return t * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))));
}

CAM_HD void cam_equi_n(const double* k, double x, double y, double* xd, double* yd) {
    const double r2 = x * x + y * y;
    const double r = sqrt(r2);
    const double theta = cam_atan(r);
    const double td = cam_equi_poly(k, theta);
    const double s = r == 0.0 ? 1.0 : td / r;
    *xd = x * s;
    *yd = y * s;
}

CAM_HD void cam_distort_n(const cam_rec& c, int model, double x, double y, double* xd, double* yd) {
    if (model == CAM_RADTAN) cam_radtan_n(c.k, x, y, xd, yd);
    else if (model == CAM_EQUIDISTANT) cam_equi_n(c.k, x, y, xd, yd);
    else { *xd = x; *yd = y; }
}

// normalised (x, y) -> raw pixel
CAM_HD void cam_project(const cam_rec& c, int model, double x, double y, double* u, double* v) {
    double xd, yd;
    cam_distort_n(c, model, x, y, &xd, &yd);
    *u = c.fx * xd + c.cx;
    *v = c.fy * yd + c.cy;
}

// pinhole pixel of the same fx..cy -> raw pixel (slam_cam_distort_f64): status 3 and NaN for an input that is not finite
CAM_HD cam_point cam_distort_px(const cam_rec& c, int model, double u, double v) {
    cam_point o;
    const double nan = __builtin_nan("");
    o.x = o.y = o.u = o.v = nan;
    o.status = CAM_NOT_FINITE;
    if (!(cam_finite(u) && cam_finite(v))) return o;
    const double x = (u - c.cx) / c.fx, y = (v - c.cy) / c.fy;
    cam_distort_n(c, model, x, y, &o.x, &o.y);
    o.u = c.fx * o.x + c.cx;
    o.v = c.fy * o.y + c.cy;
    o.status = CAM_OK;
    return o;
}

// ---- inverse ---------------------------------------------------------------------------------------------------------------
// radtan: exactly `iterations` Newton steps on cam_radtan_n(x, y) - (x0, y0) = 0 from (x0, y0), no early exit.  *fold is set
// when the (symmetric) Jacobian is not positive definite - det > 0 and trace > 0 - at an iterate a step is taken from: the
// determinant alone is positive again far beyond the fold, where both eigenvalues are negative, and a long step from just inside
// the fold can land there.  *res is max(|dx|, |dy|) at the result.
CAM_HD void cam_radtan_inverse(const double* k, double x0, double y0, int iterations, double* xo, double* yo, bool* fold, double* res) {
    const double k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4];
    double x = x0, y = y0;
    bool bad = false;
    for (int it = 0; it < iterations; it++) {
        const double r2 = x * x + y * y;
        const double rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3));
        const double dr = k1 + r2 * (2.0 * k2 + r2 * (3.0 * k3));                 // d rad / d r2
        const double ex = ((x * rad + ((2.0 * p1) * x) * y) + p2 * (r2 + (2.0 * x) * x)) - x0;
        const double ey = ((y * rad + p1 * (r2 + (2.0 * y) * y)) + ((2.0 * p2) * x) * y) - y0;
        const double xy2 = ((2.0 * x) * y) * dr;
        const double cross = xy2 + ((2.0 * p1) * x + (2.0 * p2) * y);             // d xd / d y = d yd / d x
        const double a = (rad + ((2.0 * x) * x) * dr) + ((2.0 * p1) * y + (6.0 * p2) * x);
        const double d = (rad + ((2.0 * y) * y) * dr) + ((6.0 * p1) * y + (2.0 * p2) * x);
        const double det = a * d - cross * cross;
        bad = bad || !(det > 0.0) || !(a + d > 0.0);
        x = x - (d * ex - cross * ey) / det;
        y = y - (a * ey - cross * ex) / det;
    }
    double xd, yd;
    cam_radtan_n(k, x, y, &xd, &yd);
    *res = cam_max(fabs(xd - x0), fabs(yd - y0));
    *xo = x;
    *yo = y;
    *fold = bad;
}

// equidistant: exactly `iterations` Newton steps on cam_equi_poly(theta) - rd = 0 from theta = rd.  *fold: the derivative was
// not > 0 at an iterate, or the result is not below CAM_THETA_MAX; *res = |theta_d(theta) - rd|, which bounds max(|dx|, |dy|).
CAM_HD void cam_equi_inverse(const double* k, double x0, double y0, int iterations, double* xo, double* yo, bool* fold, double* res) {
    const double rd = sqrt(x0 * x0 + y0 * y0);
    double t = rd;
    bool bad = false;
    for (int it = 0; it < iterations; it++) {
        const double t2 = t * t;
        const double f = t * (1.0 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3])))) - rd;
        const double df = 1.0 + t2 * (3.0 * k[0] + t2 * (5.0 * k[1] + t2 * (7.0 * k[2] + t2 * (9.0 * k[3]))));
        bad = bad || !(df > 0.0);
        t = t - f / df;
    }
    *res = fabs(cam_equi_poly(k, t) - rd);
    bad = bad || !(t < CAM_THETA_MAX) || !(t >= 0.0);
    const double s = rd == 0.0 ? 1.0 : cam_tan(bad ? 0.0 : t) / rd;
    *xo = x0 * s;
    *yo = y0 * s;
    *fold = bad;
}

// raw pixel -> normalised (x, y) and pinhole pixel (fx x + cx, fy y + cy), with the status of the header; NaN unless status 0
CAM_HD cam_point cam_undistort_px(const cam_rec& c, int model, double u, double v, int iterations) {
    cam_point o;
    const double nan = __builtin_nan("");
    o.x = o.y = o.u = o.v = nan;
    o.status = CAM_NOT_FINITE;
    if (!(cam_finite(u) && cam_finite(v))) return o;
    const double x0 = (u - c.cx) / c.fx, y0 = (v - c.cy) / c.fy;
    double x = x0, y = y0, res = 0.0;
    bool fold = false;
    if (model == CAM_RADTAN) cam_radtan_inverse(c.k, x0, y0, iterations, &x, &y, &fold, &res);
    else if (model == CAM_EQUIDISTANT) cam_equi_inverse(c.k, x0, y0, iterations, &x, &y, &fold, &res);
    const double tol = (64.0 * 2.220446049250313e-16) * cam_max(1.0, cam_max(fabs(x0), fabs(y0)));
    o.status = fold ? CAM_NO_IMAGE : (res <= tol ? CAM_OK : CAM_NOT_CONVERGED);
    if (o.status != CAM_OK) return o;
    o.x = x;
    o.y = y;
    o.u = c.fx * x + c.cx;
    o.v = c.fy * y + c.cy;
    return o;
}

// ---- one entry of the rectification map ------------------------------------------------------------------------------------
// destination pixel (j, i) of the camera K' = (nfx, nfy, ncx, ncy) turned by R (row-major [9]): the raw pixel in 1/32 units,
// or the sentinel pair.  Returns false for the sentinel.
CAM_HD bool cam_map_entry(const cam_rec& c, int model, const double* R, double nfx, double nfy, double ncx, double ncy, int j, int i,
                          int32_t* U, int32_t* V) {
    *U = *V = CAM_MAP_SENTINEL;
    const double xn = ((double)j - ncx) / nfx, yn = ((double)i - ncy) / nfy;
    const double X = (R[0] * xn + R[3] * yn) + R[6];
    const double Y = (R[1] * xn + R[4] * yn) + R[7];
    const double Z = (R[2] * xn + R[5] * yn) + R[8];
    if (!(Z > 0.0)) return false;
    double u, v;
    cam_project(c, model, X / Z, Y / Z, &u, &v);
    const double su = 32.0 * u, sv = 32.0 * v;
    if (!(fabs(su) < 1073741824.0 && fabs(sv) < 1073741824.0)) return false;      // (NaN and inf fail here too)
    *U = (int32_t)rint(su);
    *V = (int32_t)rint(sv);
    return true;
}

// host-side check of a record: 0 when it is finite with fx, fy > 0 and a model in {0, 1, 2}
inline int cam_record_check(const double* r) {
    for (int k = 0; k < CAM_RECORD; k++)
        if (!(fabs(r[k]) <= CAM_DBL_MAX)) return 1;
    if (!(r[0] > 0.0 && r[1] > 0.0)) return 2;
    if (!(r[4] == 0.0 || r[4] == 1.0 || r[4] == 2.0)) return 3;
    return 0;
}

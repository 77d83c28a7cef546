// Host twin of one wave for dense_cost_grad_kernel (csrc/traj_dense.hip): 64 threads in lock step at the shuffle points (publish /
// barrier / read), threadIdx.x per thread, the dynamic LDS as a 64 KB array.  The kernel text itself -- hermite_state, load_interval,
// fk_points_axes, field_forces, joint_torques and the kernel -- is the library's: tests/test_cpu_dense_grad_wave.py cuts it out of
// traj_dense.hip into kernel_funcs.inc; only the device intrinsics and the structs of cost_device.h / sgpmp_internal.h it reads are
// restated here.  Built with -fsanitize=address,undefined -ffp-contract=off; reads one case from a text file (argv[1]), prints the
// B values and the B x T x 2n gradient.
#include <pthread.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <thread>
#include <vector>
#define __device__
#define __global__
#define __forceinline__ inline
#define __launch_bounds__(x)
#define __shared__
#define __align__(x) alignas(x)
#define SGPMP_CONST
#define SGPMP_MAX_INTERP 8
#define SGPMP_MAX_JOINTS 16
#define SGPMP_MAX_DOF 8
#define SGPMP_MAX_TERMS 8
#define SGPMP_MAX_SUBSTEPS 31
enum { SGPMP_COST_SPHERES = 4, SGPMP_COST_SELF = 5 };
enum { SGPMP_FIELD_RBF = 0, SGPMP_FIELD_SDF = 1, SGPMP_FIELD_OCCUPANCY = 2 };
#define SGPMP_FLAG_SDF_CLAMP 16
static pthread_barrier_t g_bar;
static thread_local int t_lane;
struct Idx { int x; };
struct LaneIdx { operator int() const { return t_lane; } };
static struct { LaneIdx x; } threadIdx;
static Idx blockIdx = {0}, gridDim = {1};
static double g_slot[64];
static int g_islot[64];
template <typename T> static T xchg(T v, int src) {        // every lane publishes, then reads lane `src` (own value when out of range)
    static_assert(sizeof(T) <= 8, "");
    std::memcpy(&g_slot[t_lane], &v, sizeof(T));
    pthread_barrier_wait(&g_bar);
    T r = v;
    if (src >= 0 && src < 64) std::memcpy(&r, &g_slot[src], sizeof(T));
    pthread_barrier_wait(&g_bar);
    return r;
}
template <typename T> static T __shfl_down(T v, int d, int) { return xchg(v, t_lane + d); }
template <typename T> static T __shfl_up(T v, int d, int) { return xchg(v, t_lane - d); }
template <typename T> static T __shfl(T v, int s, int) { return xchg(v, s); }
template <typename T> static T __shfl_xor(T v, int m, int) { return xchg(v, t_lane ^ m); }
static int __any(int p) {
    g_islot[t_lane] = p;
    pthread_barrier_wait(&g_bar);
    int r = 0;
    for (int i = 0; i < 64; ++i) r |= g_islot[i] != 0;
    pthread_barrier_wait(&g_bar);
    return r;
}
static double wave_sum(double v) { for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64); return v; }
struct JointDev { double R[9]; double t[3]; int revolute; int qidx; };
struct ChainDev { int n_joints, n_links; JointDev j[SGPMP_MAX_JOINTS]; float Rf[SGPMP_MAX_JOINTS][9]; float tf[SGPMP_MAX_JOINTS][3]; };
typedef const ChainDev* ChainC;
template <typename T> const T* as_const(const T* p) { return p; }
template <typename T> const T* opaque(const T* p) { return p; }
template <typename real> struct RealOps;
template <> struct RealOps<float> {
    static float mul_rn(float a, float b) { return a * b; }
    static float exp_(float a) { return expf(a); } static float sqrt_(float a) { return sqrtf(a); }
    static void sincos_(float a, float* s, float* c) { *s = sinf(a); *c = cosf(a); } };
template <> struct RealOps<double> {
    static double mul_rn(double a, double b) { return a * b; }
    static double exp_(double a) { return exp(a); } static double sqrt_(double a) { return sqrt(a); }
    static void sincos_(double a, double* s, double* c) { *s = sin(a); *c = cos(a); } };
template <typename real> struct JointK;
template <> struct JointK<float> { static float R(ChainC ch, int j, int i) { return ch->Rf[j][i]; } static float t(ChainC ch, int j, int i) { return ch->tf[j][i]; } };
template <> struct JointK<double> { static double R(ChainC ch, int j, int i) { return ch->j[j].R[i]; } static double t(ChainC ch, int j, int i) { return ch->j[j].t[i]; } };
template <typename real> struct TermK {
    int kind, flags; real K, K2, dt, c11, c12, c22, selfc, inv_cell, off_x, off_y; const void* dev_data; int dim0, dim1;
    long long rows_per_goal; int n_points, n_interp, interp_lo, interp_hi; real alpha[SGPMP_MAX_INTERP]; };
alignas(16) unsigned char lds_raw[64 * 1024];

#include "kernel_funcs.inc"


template <typename real, int N, int NJ>
static void go(FILE* in, const ChainDev& ch, int T, int n_sub, double dt, int support, int accumulate, double weight, int B) {
    DenseCostK<real> A; std::memset(&A, 0, sizeof(A));
    A.T = T; A.n_sub = n_sub; A.accumulate = accumulate; A.weight = (real)weight; A.n_links = ch.n_links; A.chain = &ch;
    int nt; fscanf(in, "%d", &nt);
    for (int t = 0; t < nt; ++t) {
        double K, K2, al[8]; int kind, flags, np, ni, lo, hi;
        fscanf(in, "%d %d %lf %lf %d %d %d %d", &kind, &flags, &K, &K2, &np, &ni, &lo, &hi);
        for (int a = 0; a < 8; ++a) fscanf(in, "%lf", &al[a]);
        TermK<real>& k = A.t[A.n_terms++];
        k.kind = kind; k.flags = flags; k.K = (real)K; k.K2 = (real)K2; k.n_points = np; k.n_interp = ni; k.interp_lo = lo; k.interp_hi = hi;
        for (int a = 0; a < 8; ++a) k.alpha[a] = (real)al[a];
    }
    int ns; fscanf(in, "%d", &ns);
    std::vector<real> sph(ns * 4);
    for (auto& v : sph) { double d; fscanf(in, "%lf", &d); v = (real)d; }
    A.spheres = ns ? sph.data() : nullptr; A.n_spheres = ns;
    int hq, hv; double sig; fscanf(in, "%d %d %lf", &hq, &hv, &sig);
    const real inf = std::numeric_limits<real>::infinity();
    A.has_qlim = hq; A.has_vlim = hv; A.inv_sigma2 = (hq | hv) ? (real)(1. / (sig * sig)) : 0;
    for (int k = 0; k < SGPMP_MAX_DOF; ++k) { A.q_lo[k] = -inf; A.q_hi[k] = inf; A.v_max[k] = inf; }
    for (int k = 0; k < N && hq; ++k) { double lo, hi; fscanf(in, "%lf %lf", &lo, &hi); A.q_lo[k] = (real)lo; A.q_hi[k] = (real)hi; }
    for (int k = 0; k < N && hv; ++k) { double v; fscanf(in, "%lf", &v); A.v_max[k] = (real)v; }
    std::vector<real> x((size_t)B * T * 2 * N), g((size_t)B * T * 2 * N);
    for (auto& v : x) { double d; fscanf(in, "%lf", &d); v = (real)d; }
    for (auto& v : g) { double d; fscanf(in, "%lf", &d); v = (real)d; }       // what grad holds before the call
    std::vector<double> c64(B);
    const HermiteK<real> H = hermite_coefs<real>(n_sub, dt);
    pthread_barrier_init(&g_bar, nullptr, 64);
    std::vector<std::thread> th;
    for (int l = 0; l < 64; ++l)
        th.emplace_back([&, l] { t_lane = l; dense_cost_grad_kernel<real, N, NJ>(x.data(), (long long)B, A, H, support, g.data(), (real*)nullptr, c64.data()); });
    for (auto& t : th) t.join();
    for (int b = 0; b < B; ++b) printf("%.17g\n", c64[b]);
    for (auto v : g) printf("%.17g\n", (double)v);
}

int main(int argc, char** argv) {
    FILE* in = fopen(argv[1], "r");
    int dtype, njf, n, nj, T, n_sub, support, accumulate, B; double dt, weight;
    fscanf(in, "%d %d %d %d %d %d %lf %d %d %lf %d", &dtype, &njf, &n, &nj, &T, &n_sub, &dt, &support, &accumulate, &weight, &B);
    ChainDev ch = {}; ch.n_joints = nj; ch.n_links = nj + 1;
    for (int j = 0; j < nj; ++j) {
        for (int i = 0; i < 9; ++i) { fscanf(in, "%lf", &ch.j[j].R[i]); ch.Rf[j][i] = (float)ch.j[j].R[i]; }
        for (int i = 0; i < 3; ++i) { fscanf(in, "%lf", &ch.j[j].t[i]); ch.tf[j][i] = (float)ch.j[j].t[i]; }
        fscanf(in, "%d %d", &ch.j[j].revolute, &ch.j[j].qidx);
    }
#define GO(R_, N_, NJ_) go<R_, N_, NJ_>(in, ch, T, n_sub, dt, support, accumulate, weight, B)
    if (n == 7 && njf == 10) { if (dtype) GO(double, 7, 10); else GO(float, 7, 10); }
    else if (n == 7 && njf == 0) { if (dtype) GO(double, 7, 0); else GO(float, 7, 0); }
    else if (n == 2) { if (dtype) GO(double, 2, -1); else GO(float, 2, -1); }
    return 0;
}

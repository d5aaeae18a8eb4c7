// Diagnostic micro-benchmark (not part of the product): what does one packed FP32 instruction (v_pk_add_f32 / v_pk_mul_f32) cost
// against one scalar one (v_add_f32 / v_mul_f32) on MI355X, at the record step's occupancy (4 waves per SIMD, every CU busy)?
//   hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fno-slp-vectorize tools/pkissue.hip -o pkissue;  ./pkissue [trips [waves per SIMD, 1..4]]
// -fno-slp-vectorize keeps the scalar arm scalar (the packed arm is written in the two-float ext-vector type and does not depend on
// SLP). Both arms run the same NUMBER of vector instructions, in 16, 4, 2 or 1 independent chains per lane, so a packed instruction
// does twice the arithmetic of a scalar one. What is reported is time per instruction, as SIMD cycles at the device's clock:
// elapsed * clock / (instructions per wave * waves per SIMD). Result on MI355X: profiles/packed_f32_issue_cost.txt.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <vector>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(1); } } while (0)

typedef float float2v __attribute__((ext_vector_type(2)));

constexpr int PER_TRIP = 128;   // vector instructions per loop trip, against one s_add + s_cmp + s_cbranch
constexpr int MAX_WAVES_PER_SIMD = 4;

template <class T> __device__ __forceinline__ T splat(float a, float b);
template <> __device__ __forceinline__ float splat<float>(float a, float) { return a; }
template <> __device__ __forceinline__ float2v splat<float2v>(float a, float b) { return float2v{a, b}; }
__device__ __forceinline__ float fold(float v) { return v; }
__device__ __forceinline__ float fold(float2v v) { return v.x + v.y; }

// MUL = false: acc += c; MUL = true: acc *= c (c = 1 + 2^-20: the product stays finite and never becomes a constant)
// CHAINS independent accumulators per lane (CHAINS or 2 CHAINS VGPRs), each advanced PER_TRIP / CHAINS times per trip: 16 chains
// measure issue alone, 1 or 2 chains what a wave waits for a dependent result while three other waves share the SIMD
template <class T, bool MUL, int CHAINS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MAX_WAVES_PER_SIMD, MAX_WAVES_PER_SIMD))) void k_chain(float *out, float c0, float c1, int trips)
{
    T acc[CHAINS];
#pragma unroll
    for (int i = 0; i < CHAINS; ++i) acc[i] = splat<T>((float)(threadIdx.x + i), (float)(i + 1));
    const T c = splat<T>(c0, c1);
    for (int t = 0; t < trips; ++t) {
#pragma unroll
        for (int u = 0; u < PER_TRIP / CHAINS; ++u) {
#pragma unroll
            for (int i = 0; i < CHAINS; ++i) acc[i] = MUL ? acc[i] * c : acc[i] + c;
        }
    }
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < CHAINS; ++i) s += fold(acc[i]);
    out[(size_t)blockIdx.x * blockDim.x + threadIdx.x] = s;
}

template <class T, bool MUL, int CHAINS>
static double time_arm(float *out, int grid, int trips, float c0, float c1)
{
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int rep = 0; rep < 7; ++rep) {      // the first two are warm-up
        CK(hipEventRecord(e0));
        k_chain<T, MUL, CHAINS><<<grid, 256>>>(out, c0, c1, trips);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
        float t; CK(hipEventElapsedTime(&t, e0, e1));
        if (rep >= 2) ms.push_back(t);
    }
    CK(hipGetLastError());
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    std::sort(ms.begin(), ms.end());
    return ms[ms.size() / 2];
}

template <int CHAINS>
static void report(float *out, int grid, int waves, int trips, double mhz, double instr)
{
    const float m0 = 1.0f + 0x1p-20f, m1 = 1.0f - 0x1p-20f;
    struct { const char *name; double ms; } arm[4];
    arm[0] = {"v_add_f32   ", time_arm<float, false, CHAINS>(out, grid, trips, 1.0f, 2.0f)};
    arm[1] = {"v_pk_add_f32", time_arm<float2v, false, CHAINS>(out, grid, trips, 1.0f, 2.0f)};
    arm[2] = {"v_mul_f32   ", time_arm<float, true, CHAINS>(out, grid, trips, m0, m1)};
    arm[3] = {"v_pk_mul_f32", time_arm<float2v, true, CHAINS>(out, grid, trips, m0, m1)};
    for (int a = 0; a < 4; ++a) {
        const double cyc = arm[a].ms * 1e-3 * mhz * 1e6 / (instr * waves);
        printf("%6d | %s | %10.4f       | %8.3f                    | %6.2f\n", CHAINS, arm[a].name, arm[a].ms, cyc, 64.0 * ((a & 1) ? 2 : 1) / cyc);
    }
    printf("%6d | packed / scalar: add %.3f, mul %.3f\n", CHAINS, arm[1].ms / arm[0].ms, arm[3].ms / arm[2].ms);
}

int main(int argc, char **argv)
{
    const int trips = argc > 1 ? atoi(argv[1]) : 20000;
    const int waves = argc > 2 ? std::min(std::max(atoi(argv[2]), 1), MAX_WAVES_PER_SIMD) : MAX_WAVES_PER_SIMD;      // waves per SIMD
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    const double mhz = prop.clockRate / 1000.0;      // kHz -> MHz
    const int grid = cus * waves;                    // 4 waves per workgroup = one per SIMD; `waves` workgroups per CU
    float *out;
    CK(hipMalloc(&out, (size_t)grid * 256 * sizeof(float)));
    const double instr = (double)trips * PER_TRIP;      // per wave
    printf("%s: %d CUs, clock %.0f MHz, %d workgroups of 256 (%d waves per SIMD), %.0f vector instructions per wave\n", prop.gcnArchName, cus, mhz, grid,
           waves, instr);
    printf("chains | instruction  | ms (median of 5) | SIMD cycles per instruction | f32 operations per SIMD cycle\n");
    report<16>(out, grid, waves, trips, mhz, instr);
    report<4>(out, grid, waves, trips, mhz, instr);
    report<2>(out, grid, waves, trips, mhz, instr);
    report<1>(out, grid, waves, trips, mhz, instr);
    CK(hipFree(out));
    return 0;
}

/*
 * Symmetric Gauss-Seidel as a solver through spgpu/ext/sweep_device.h, written against the C ABI only.  A is the 7-point Laplacian
 * on a g^3 grid with the diagonal 6 + (i % 3) / 4 (symmetric, diagonally dominant), held WHOLE in CSR in its natural order, as in
 * tools/gs_amd.c and tools/multicolour_amd.c.
 *
 *   (a) A is coloured and the rows are listed colour by colour (spgpu/ext/colour_device.h); spgpuCsrSweepPlanDevice checks the
 *       colouring against the stored entries and finds the diagonals;
 *   (b) one symmetric sweep from x = 0 on A ITSELF -- no permuted copy, no gathered vector -- is compared BIT FOR BIT with a
 *       restatement in plain C: colours 0 .. C-1 and back, every row's differences in storage order, each product rounded on its own;
 *   (c) symmetric sweeps go on until spgpuCsrResidualDevice and spgpuDnrm2 report ||b - A x|| / ||b|| <= tol, the bound of gs_amd.
 *
 *   usage: sweep_amd [grid=8] [maxSweeps=2000] [tol=1e-8]
 * Prints the sweeps, the colours and the launches of one sweep (a colour of more than 256 rows is a launch, a run of narrower
 * colours one launch per 64 of them, forwards and backwards).  Exits 0 iff (b) matches and (c) converged, with the residual
 * recomputed on the host within 10 tol.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/vector.h"
#include "spgpu/ext/colour_device.h"
#include "spgpu/ext/sweep_device.h"

#define CHECK(call)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)
#define OK(call)                                                                  \
    do {                                                                          \
        if ((call) != SPGPU_SUCCESS) {                                            \
            fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #call);     \
            exit(2);                                                              \
        }                                                                         \
    } while (0)

enum { CHAIN_WIDTH = 256, CHAIN_PASSES = 64 };

/* one colour pass of the contract on the host; the volatile keeps the product rounded on its own whatever the compiler fuses */
static void hostPass(double* x, const double* b, const int* order, int begin, int end, const int* diagPos, const int* ptr, const int* idx,
                     const double* val)
{
    for (int t = begin; t < end; ++t) {
        const int i = order[t];
        double acc = b[i];
        for (int e = ptr[i]; e < ptr[i + 1]; ++e)
            if (e != diagPos[i]) {
                volatile double product = val[e] * x[idx[e]];
                acc = acc - product;
            }
        x[i] = acc / val[diagPos[i]];
    }
}

/* the launches of one list of colours, visited in the given direction */
static int launchesOf(const int* colourPtr, int colours, int step)
{
    int launches = 0, run = 0;
    for (int k = 0; k < colours; ++k) {
        const int c = step > 0 ? k : colours - 1 - k;
        if (colourPtr[c + 1] - colourPtr[c] > CHAIN_WIDTH) {
            launches += (run + CHAIN_PASSES - 1) / CHAIN_PASSES + 1;
            run = 0;
        } else {
            ++run;
        }
    }
    return launches + (run + CHAIN_PASSES - 1) / CHAIN_PASSES;
}

int main(int argc, char** argv)
{
    const int g = argc > 1 ? atoi(argv[1]) : 8;
    const int maxSweeps = argc > 2 ? atoi(argv[2]) : 2000;
    const double tol = argc > 3 ? atof(argv[3]) : 1e-8;
    if (g < 2 || g > 1000 || maxSweeps < 1) {
        fprintf(stderr, "usage: sweep_amd [grid=8] [maxSweeps=2000] [tol=1e-8]\n");
        return 2;
    }
    const int n = g * g * g;

    /* A in CSR (base 0, columns ascending) */
    int nnz = 0;
    int* ptr = (int*)malloc(((size_t)n + 1) * sizeof(int));
    int* idx = (int*)malloc((size_t)7 * n * sizeof(int));
    double* val = (double*)malloc((size_t)7 * n * sizeof(double));
#define ENTRY(j, v) { idx[nnz] = (j); val[nnz++] = (v); }
    for (int i = 0; i < n; ++i) {
        const int gx = i % g, gy = (i / g) % g, gz = i / (g * g);
        ptr[i] = nnz;
        if (gz > 0)     ENTRY(i - g * g, -1.0)
        if (gy > 0)     ENTRY(i - g, -1.0)
        if (gx > 0)     ENTRY(i - 1, -1.0)
        ENTRY(i, 6.0 + (i % 3) * 0.25)
        if (gx < g - 1) ENTRY(i + 1, -1.0)
        if (gy < g - 1) ENTRY(i + g, -1.0)
        if (gz < g - 1) ENTRY(i + g * g, -1.0)
    }
#undef ENTRY
    ptr[n] = nnz;
    /* b = A * xTrue, xTrue_i = 1 + (i % 7) / 8 */
    double* b = (double*)calloc(n, sizeof(double));
    for (int i = 0; i < n; ++i)
        for (int e = ptr[i]; e < ptr[i + 1]; ++e)
            b[i] += val[e] * (1.0 + (idx[e] % 7) * 0.125);

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS) return 2;
    hipStream_t stream = spgpuGetStream(h);
    const size_t vecBytes = (size_t)n * sizeof(double);
    int *dPtr, *dIdx, *dColourOf, *dOrder, *dInverse, *dColourPtr, *dDiagPos;
    double *dVal, *dB, *dX, *dR;
    void *work, *sweepWork;
    CHECK(hipMalloc((void**)&dPtr, ((size_t)n + 1) * sizeof(int)));
    CHECK(hipMalloc((void**)&dIdx, (size_t)nnz * sizeof(int)));
    CHECK(hipMalloc((void**)&dVal, (size_t)nnz * sizeof(double)));
    CHECK(hipMalloc((void**)&dB, vecBytes));
    CHECK(hipMalloc((void**)&dX, vecBytes));
    CHECK(hipMalloc((void**)&dR, vecBytes));
    CHECK(hipMemcpy(dPtr, ptr, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dIdx, idx, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dVal, val, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dB, b, vecBytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(dX, 0, vecBytes));

    /* ---- (a) colour, order, plan ---- */
    int colours = 0, rounds = 0, entries = 0;
    CHECK(hipMalloc((void**)&dColourOf, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&dOrder, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&dInverse, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&dDiagPos, (size_t)n * sizeof(int)));
    CHECK(hipMalloc(&work, spgpuCsrColourWorkBytes(n)));
    CHECK(hipMalloc(&sweepWork, spgpuCsrSweepWorkBytes(n)));
    OK(spgpuCsrColourDevice(h, &colours, &rounds, dColourOf, n, dPtr, dIdx, 0, work));
    CHECK(hipMalloc((void**)&dColourPtr, ((size_t)colours + 1) * sizeof(int)));
    OK(spgpuCsrColourOrderDevice(h, dOrder, dInverse, dColourPtr, n, colours, dColourOf, work));
    int* colourPtrHost = (int*)malloc(((size_t)colours + 1) * sizeof(int));
    OK(spgpuCsrSweepPlanDevice(h, &entries, dDiagPos, colourPtrHost, n, colours, dOrder, dColourPtr, dColourOf, dPtr, dIdx, 0, sweepWork));
    CHECK(hipFree(sweepWork));
    const int launches = launchesOf(colourPtrHost, colours, 1) + launchesOf(colourPtrHost, colours, -1);

    /* ---- (b) the first sweep against the host ---- */
#define SWEEP() \
    OK(spgpuCsrSweepDevice(h, dX, dB, n, colours, dOrder, colourPtrHost, dDiagPos, dPtr, dIdx, dVal, 0, SPGPU_SWEEP_SYMMETRIC, NULL, \
                           SPGPU_TYPE_DOUBLE, entries))
    SWEEP();
    CHECK(hipStreamSynchronize(stream));
    int* order = (int*)malloc((size_t)n * sizeof(int));
    int* diagPos = (int*)malloc((size_t)n * sizeof(int));
    double* x = (double*)malloc(vecBytes);
    double* xHost = (double*)calloc(n, sizeof(double));
    CHECK(hipMemcpy(order, dOrder, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(diagPos, dDiagPos, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(x, dX, vecBytes, hipMemcpyDeviceToHost));
    int planSound = entries == nnz;
    for (int i = 0; i < n; ++i)
        planSound = planSound && diagPos[i] >= ptr[i] && diagPos[i] < ptr[i + 1] && idx[diagPos[i]] == i;
    if (planSound) {
        for (int c = 0; c < colours; ++c)
            hostPass(xHost, b, order, colourPtrHost[c], colourPtrHost[c + 1], diagPos, ptr, idx, val);
        for (int c = colours - 1; c >= 0; --c)
            hostPass(xHost, b, order, colourPtrHost[c], colourPtrHost[c + 1], diagPos, ptr, idx, val);
    }
    const int sameBytes = planSound && memcmp(x, xHost, vecBytes) == 0;

    /* ---- (c) sweeps until the residual is small ---- */
    const double bNorm = spgpuDnrm2(h, n, dB);
    int sweeps = 1;
    OK(spgpuCsrResidualDevice(h, dR, dB, dX, n, dPtr, dIdx, dVal, 0, SPGPU_TYPE_DOUBLE, entries));
    double relative = spgpuDnrm2(h, n, dR) / bNorm;
    while (sweeps < maxSweeps && relative > tol) {
        SWEEP();
        ++sweeps;
        OK(spgpuCsrResidualDevice(h, dR, dB, dX, n, dPtr, dIdx, dVal, 0, SPGPU_TYPE_DOUBLE, entries));
        relative = spgpuDnrm2(h, n, dR) / bNorm;
    }
#undef SWEEP
    CHECK(hipStreamSynchronize(stream));
    CHECK(hipMemcpy(x, dX, vecBytes, hipMemcpyDeviceToHost));
    double rr = 0, bb = 0;
    for (int i = 0; i < n; ++i) {
        double r = b[i];
        for (int e = ptr[i]; e < ptr[i + 1]; ++e)
            r -= val[e] * x[idx[e]];
        rr += r * r;
        bb += b[i] * b[i];
    }
    const double hostRelative = sqrt(rr / bb);
    const int converged = relative <= tol && hostRelative <= 10 * tol;

    printf("symmetric Gauss-Seidel on a %d^3 grid (%d rows, %d nnz): %d colours in %d rounds, %d launches a sweep, first sweep %s\n", g, n,
           nnz, colours, rounds, launches, sameBytes ? "equal to the host's bit for bit" : "DIFFERS from the host's");
    printf("%d sweeps, ||b - A x|| / ||b|| = %.3e on the device, %.3e on the host (%s)\n", sweeps, relative, hostRelative,
           converged ? "converged" : "NOT converged");
    const int passed = sameBytes && converged;
    printf("%s\n", passed ? "PASSED" : "FAILED");

    CHECK(hipFree(dPtr)); CHECK(hipFree(dIdx)); CHECK(hipFree(dVal)); CHECK(hipFree(dB)); CHECK(hipFree(dX)); CHECK(hipFree(dR));
    CHECK(hipFree(dColourOf)); CHECK(hipFree(dOrder)); CHECK(hipFree(dInverse)); CHECK(hipFree(dColourPtr)); CHECK(hipFree(dDiagPos));
    CHECK(hipFree(work));
    free(ptr); free(idx); free(val); free(b); free(colourPtrHost); free(order); free(diagPos); free(x); free(xHost);
    spgpuDestroy(h);
    return passed ? 0 : 1;
}

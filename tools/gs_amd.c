/*
 * Gauss-Seidel through the sparse triangular solve of spgpu/ext/trsv_device.h, written against the C ABI only.  A is the 5-point
 * Laplacian on a g x g grid with the diagonal 4 + (i % 3) / 4 (symmetric, diagonally dominant), held WHOLE in CSR; both triangles
 * are solved from A's own arrays.
 *
 *   (a) one forward solve (D + L)^-1 b and one backward solve (D + U)^-1 b, each compared BIT FOR BIT with a substitution in plain
 *       C that follows the header's contract (product rounded, then the difference; one division);
 *   (b) CG preconditioned by symmetric Gauss-Seidel, z = (D + U)^-1 D (D + L)^-1 r: two spgpuCsrTrsvDevice calls and one spgpuDaxy
 *       per iteration, spgpuDhellspmv / spgpuDdot / spgpuDaxpby for the rest;
 *   (c) plain CG on the same system to the same relative residual.
 *
 *   usage: gs_amd [grid=64] [maxIter=2000] [tol=1e-8]
 * Exits 0 iff both solves of (a) match, (b) converged, and (b) needed fewer iterations than (c).
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/ell_conv.h"
#include "spgpu/hell.h"
#include "spgpu/hell_conv.h"
#include "spgpu/vector.h"
#include "spgpu/ext/trsv_device.h"

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

/* the contract on the host: rows ascending (lower) or descending (upper); volatile keeps the product from being fused */
static void substitute(double* x, const double* b, int n, const int* ptr, const int* idx, const double* val, int lower)
{
    for (int s = 0; s < n; ++s) {
        const int i = lower ? s : n - 1 - s;
        double acc = b[i], pivot = 0.0;
        for (int e = ptr[i]; e < ptr[i + 1]; ++e) {
            const int j = idx[e];
            if (j == i) {
                pivot = val[e];
            } else if (lower ? j < i : j > i) {
                volatile double product = val[e] * x[j];
                acc = acc - product;
            }
        }
        x[i] = acc / pivot;
    }
}

typedef struct {
    int levels;
    int *order, *levelPtr, *levelPtrHost;
} Plan;

static Plan makePlan(spgpuHandle_t h, int n, const int* dPtr, const int* dIdx, int side)
{
    Plan p;
    void* work;
    CHECK(hipMalloc((void**)&p.order, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&p.levelPtr, ((size_t)n + 1) * sizeof(int)));
    p.levelPtrHost = (int*)malloc(((size_t)n + 1) * sizeof(int));
    CHECK(hipMalloc(&work, spgpuCsrTrsvWorkBytes(n)));
    OK(spgpuCsrTrsvPlanDevice(h, &p.levels, p.order, p.levelPtr, p.levelPtrHost, n, dPtr, dIdx, 0, side, SPGPU_TRSV_DIAG_STORED, work));
    CHECK(hipFree(work)); /* the solve never reads it */
    return p;
}

int main(int argc, char** argv)
{
    const int g = argc > 1 ? atoi(argv[1]) : 64;
    const int maxIter = argc > 2 ? atoi(argv[2]) : 2000;
    const double tol = argc > 3 ? atof(argv[3]) : 1e-8;
    if (g < 2 || maxIter < 1) {
        fprintf(stderr, "usage: gs_amd [grid=64] [maxIter=2000] [tol=1e-8]\n");
        return 2;
    }
    const int n = g * g, hackSize = 32;

    /* A in CSR (base 0, columns ascending) and, for the SpMV, in COO -> ELL -> HELL */
    int nnz = 0;
    int* ptr = (int*)malloc(((size_t)n + 1) * sizeof(int));
    int* cr = (int*)malloc((size_t)5 * n * sizeof(int));
    int* cc = (int*)malloc((size_t)5 * n * sizeof(int));
    double* cv = (double*)malloc((size_t)5 * n * sizeof(double));
    double* diagonal = (double*)malloc((size_t)n * sizeof(double));
#define ENTRY(j, v) { cr[nnz] = i; cc[nnz] = (j); cv[nnz++] = (v); }
    for (int i = 0; i < n; ++i) {
        const int gx = i % g, gy = i / g;
        ptr[i] = nnz;
        diagonal[i] = 4.0 + (i % 3) * 0.25;
        if (gy > 0)     ENTRY(i - g, -1.0)
        if (gx > 0)     ENTRY(i - 1, -1.0)
        ENTRY(i, diagonal[i])
        if (gx < g - 1) ENTRY(i + 1, -1.0)
        if (gy < g - 1) ENTRY(i + g, -1.0)
    }
#undef ENTRY
    ptr[n] = nnz;
    int maxRow = 0, height = 0;
    int* rowLen = (int*)malloc((size_t)n * sizeof(int));
    computeEllRowLenghts(rowLen, &maxRow, n, nnz, cr, 0);
    const int pitch = computeEllAllocPitch(n);
    double* ev = (double*)calloc((size_t)maxRow * pitch, sizeof(double));
    int* ei = (int*)calloc((size_t)maxRow * pitch, sizeof(int));
    cooToEll(ev, ei, pitch, pitch, maxRow, 0, n, nnz, cr, cc, cv, 0, SPGPU_TYPE_DOUBLE);
    computeHellAllocSize(&height, hackSize, n, rowLen);
    const int hacks = (n + hackSize - 1) / hackSize;
    double* hv = (double*)calloc((size_t)hackSize * height, sizeof(double));
    int* hi = (int*)calloc((size_t)hackSize * height, sizeof(int));
    int* ho = (int*)calloc(hacks, sizeof(int));
    ellToHell(hv, hi, ho, hackSize, ev, ei, pitch, pitch, rowLen, n, SPGPU_TYPE_DOUBLE);

    /* b = A * xTrue, xTrue_i = 1 + (i % 7) / 8 */
    double* b = (double*)calloc(n, sizeof(double));
    for (int e = 0; e < nnz; ++e)
        b[cr[e]] += cv[e] * (1.0 + (cc[e] % 7) * 0.125);

    const size_t vecBytes = (size_t)n * sizeof(double);
    double *dV, *dX, *dR, *dP, *dAp, *dZ, *dT, *dD, *dVal;
    int *dI, *dHo, *dRs, *dPtr, *dIdx;
    CHECK(hipMalloc((void**)&dV, (size_t)hackSize * height * sizeof(double)));
    CHECK(hipMalloc((void**)&dI, (size_t)hackSize * height * sizeof(int)));
    CHECK(hipMalloc((void**)&dHo, hacks * sizeof(int)));
    CHECK(hipMalloc((void**)&dRs, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&dPtr, ((size_t)n + 1) * sizeof(int)));
    CHECK(hipMalloc((void**)&dIdx, (size_t)nnz * sizeof(int)));
    CHECK(hipMalloc((void**)&dVal, (size_t)nnz * sizeof(double)));
    CHECK(hipMalloc((void**)&dX, vecBytes));
    CHECK(hipMalloc((void**)&dR, vecBytes));
    CHECK(hipMalloc((void**)&dP, vecBytes));
    CHECK(hipMalloc((void**)&dAp, vecBytes));
    CHECK(hipMalloc((void**)&dZ, vecBytes));
    CHECK(hipMalloc((void**)&dT, vecBytes));
    CHECK(hipMalloc((void**)&dD, vecBytes));
    CHECK(hipMemcpy(dV, hv, (size_t)hackSize * height * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dI, hi, (size_t)hackSize * height * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dHo, ho, hacks * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dRs, rowLen, (size_t)n * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dPtr, ptr, ((size_t)n + 1) * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dIdx, cc, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dVal, cv, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dD, diagonal, vecBytes, hipMemcpyHostToDevice));

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS) return 2;
    hipStream_t stream = spgpuGetStream(h);
    const Plan lower = makePlan(h, n, dPtr, dIdx, SPGPU_TRSV_LOWER), upper = makePlan(h, n, dPtr, dIdx, SPGPU_TRSV_UPPER);
    printf("Gauss-Seidel on the %d x %d 5-point Laplacian (%d rows, %d nnz): %d levels below the diagonal, %d above\n", g, g, n, nnz,
           lower.levels, upper.levels);
#define SOLVE(plan, side, out, in) \
    OK(spgpuCsrTrsvDevice(h, out, in, n, (plan).levels, (plan).order, (plan).levelPtr, (plan).levelPtrHost, dPtr, dIdx, dVal, 0, side, \
                          SPGPU_TRSV_DIAG_STORED, SPGPU_TYPE_DOUBLE))

    /* ---- (a) both solves against the substitution, bit for bit ---- */
    double* want = (double*)malloc(vecBytes);
    double* got = (double*)malloc(vecBytes);
    int solvesMatch = 1;
    CHECK(hipMemcpy(dR, b, vecBytes, hipMemcpyHostToDevice));
    for (int backward = 0; backward < 2; ++backward) {
        substitute(want, b, n, ptr, cc, cv, !backward);
        if (backward)
            SOLVE(upper, SPGPU_TRSV_UPPER, dZ, dR);
        else
            SOLVE(lower, SPGPU_TRSV_LOWER, dZ, dR);
        CHECK(hipStreamSynchronize(stream));
        CHECK(hipMemcpy(got, dZ, vecBytes, hipMemcpyDeviceToHost));
        int differ = 0;
        double sum = 0;
        for (int i = 0; i < n; ++i) {
            differ += memcmp(&want[i], &got[i], sizeof(double)) != 0;
            sum += got[i];
        }
        printf("%s solve: %s the substitution in C (%d of %d differ), sum %.17g\n", backward ? "backward" : "forward",
               differ ? "DIFFERS from" : "equal to", differ, n, sum);
        solvesMatch &= differ == 0;
    }

    /* ---- (b) CG preconditioned by symmetric Gauss-Seidel ---- */
#define PRECONDITION()                                   \
    do {                                                 \
        SOLVE(lower, SPGPU_TRSV_LOWER, dT, dR);          \
        spgpuDaxy(h, dT, n, 1.0, dD, dT);                \
        SOLVE(upper, SPGPU_TRSV_UPPER, dZ, dT);          \
    } while (0)
    CHECK(hipMemcpy(dR, b, vecBytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(dX, 0, vecBytes));
    PRECONDITION();
    CHECK(hipMemcpyAsync(dP, dZ, vecBytes, hipMemcpyDeviceToDevice, stream));
    double rz = spgpuDdot(h, n, dR, dZ);
    double rr = spgpuDdot(h, n, dR, dR);
    const double rr0 = rr;
    int it = 0;
    while (it < maxIter && sqrt(rr / rr0) > tol) {
        spgpuDhellspmv(h, dAp, dAp, 1.0, dV, dI, hackSize, dHo, dRs, NULL, maxRow, n, dP, 0.0, 0);
        const double alpha = rz / spgpuDdot(h, n, dP, dAp);
        spgpuDaxpby(h, dX, n, 1.0, dX, alpha, dP);
        spgpuDaxpby(h, dR, n, 1.0, dR, -alpha, dAp);
        PRECONDITION();
        const double rzNew = spgpuDdot(h, n, dR, dZ);
        rr = spgpuDdot(h, n, dR, dR);
        spgpuDaxpby(h, dP, n, rzNew / rz, dP, 1.0, dZ);
        rz = rzNew;
        ++it;
    }
    const int converged = sqrt(rr / rr0) <= tol;
    CHECK(hipMemcpy(got, dX, vecBytes, hipMemcpyDeviceToHost));
    double err = 0;
    for (int i = 0; i < n; ++i) {
        const double d = fabs(got[i] - (1.0 + (i % 7) * 0.125));
        err = d > err ? d : err;
    }
    printf("SGS-PCG: %d iterations, relative residual %.3e (%s), max |x - xTrue| = %.3e\n", it, sqrt(rr / rr0),
           converged ? "converged" : "NOT converged", err);

    /* ---- (c) plain CG to the same relative residual ---- */
    CHECK(hipMemcpy(dR, b, vecBytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dP, b, vecBytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(dX, 0, vecBytes));
    double cr2 = spgpuDdot(h, n, dR, dR);
    int cgIt = 0;
    while (cgIt < maxIter && sqrt(cr2 / rr0) > tol) {
        spgpuDhellspmv(h, dAp, dAp, 1.0, dV, dI, hackSize, dHo, dRs, NULL, maxRow, n, dP, 0.0, 0);
        const double alpha = cr2 / spgpuDdot(h, n, dP, dAp);
        spgpuDaxpby(h, dX, n, 1.0, dX, alpha, dP);
        spgpuDaxpby(h, dR, n, 1.0, dR, -alpha, dAp);
        const double next = spgpuDdot(h, n, dR, dR);
        spgpuDaxpby(h, dP, n, next / cr2, dP, 1.0, dR);
        cr2 = next;
        ++cgIt;
    }
    printf("plain CG: %d iterations, relative residual %.3e\n", cgIt, sqrt(cr2 / rr0));

    spgpuDestroy(h);
    CHECK(hipGetLastError());
    const int ok = solvesMatch && converged && it < cgIt;
    printf(ok ? "PASSED\n" : "FAILED (a solve differs from the substitution, SGS-PCG did not converge, or it needed as many iterations as CG)\n");
    return ok ? 0 : 1;
}

/*
 * Jacobi-preconditioned conjugate gradient written against the C ABI only (spgpu/ext/precond.h), on a matrix plain CG cannot
 * handle: A = S L S, L the 5-point Laplacian on a g x g grid, S = diag(s_i), s_i = 10^(3 u_i - 1.5) with u_i uniform in [0, 1) --
 * a diagonal spread over three orders of magnitude, which Jacobi takes out again.  x0 = 0, b = A * ones.
 *
 * Three legs:
 *   (a) eager PCG with host scalars: spgpuDhellspmv, spgpuDdot, spgpuDaxpby, spgpuDaxy;
 *   (b) the same iterations as one captured graph per iteration from spgpuDhellspmvDotDevice, spgpuDaxpbyPairAxyDotDevice and
 *       spgpuDaxpbyQuotDevice -- 5 kernels, as many as plain CG --, two pairs of (r.z, |r|^2) cells that alternate; x, r.z and
 *       |r|^2 must come out bit for bit as in (a);
 *   (c) plain eager CG on the same matrix for maxIter iterations, for the relative residual it reaches.
 * dinv = 1 / diag(A) comes from spgpuDhellDiag(..., invert = 1) and must EQUAL 1 / ((s_i * 4) * s_i) computed on the host.
 *
 *   usage: pcg_amd [grid=32] [maxIter=200] [tol=1e-8]
 * Exits 0 iff (a) reached the tolerance, (b) is bit-identical and dinv matched.
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
#include "spgpu/device_scalars.h"
#include "spgpu/ext/precond.h"

#define CHECK(call)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)

/* a small linear congruential generator (Numerical Recipes' constants): u in [0, 1) from the upper 24 bits */
static unsigned lcgState = 12345u;
static double lcgUniform(void)
{
    lcgState = lcgState * 1664525u + 1013904223u;
    return (double)(lcgState >> 8) / 16777216.0;
}

int main(int argc, char** argv)
{
    const int g = argc > 1 ? atoi(argv[1]) : 32;
    const int maxIter = argc > 2 ? atoi(argv[2]) : 200;
    const double tol = argc > 3 ? atof(argv[3]) : 1e-8;
    if (g < 2 || maxIter < 1) {
        fprintf(stderr, "usage: pcg_amd [grid=32] [maxIter=200] [tol=1e-8]\n");
        return 2;
    }
    const int n = g * g, hackSize = 32;

    double* scale = (double*)malloc((size_t)n * sizeof(double));
    for (int i = 0; i < n; ++i)
        scale[i] = pow(10.0, 3.0 * lcgUniform() - 1.5);

    /* A = S L S in COO, natural order: entry (i, j) = (s_i * L_ij) * s_j */
    int nnz = 0;
    int* cr = (int*)malloc((size_t)5 * n * sizeof(int));
    int* cc = (int*)malloc((size_t)5 * n * sizeof(int));
    double* cv = (double*)malloc((size_t)5 * n * sizeof(double));
#define ENTRY(j, l) { cr[nnz] = i; cc[nnz] = (j); cv[nnz++] = (scale[i] * (l)) * scale[j]; }
    for (int i = 0; i < n; ++i) {
        const int gx = i % g, gy = i / g;
        if (gy > 0)     ENTRY(i - g, -1.0)
        if (gx > 0)     ENTRY(i - 1, -1.0)
        ENTRY(i, 4.0)
        if (gx < g - 1) ENTRY(i + 1, -1.0)
        if (gy < g - 1) ENTRY(i + g, -1.0)
    }
#undef ENTRY
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

    const size_t vecBytes = (size_t)n * sizeof(double);
    double *dV, *dX, *dR, *dP, *dAp, *dZ, *dDinv;
    int *dI, *dHo, *dRs;
    CHECK(hipMalloc((void**)&dV, (size_t)hackSize * height * sizeof(double)));
    CHECK(hipMalloc((void**)&dI, (size_t)hackSize * height * sizeof(int)));
    CHECK(hipMalloc((void**)&dHo, hacks * sizeof(int)));
    CHECK(hipMalloc((void**)&dRs, (size_t)n * sizeof(int)));
    CHECK(hipMalloc((void**)&dX, vecBytes));
    CHECK(hipMalloc((void**)&dR, vecBytes));
    CHECK(hipMalloc((void**)&dP, vecBytes));
    CHECK(hipMalloc((void**)&dAp, vecBytes));
    CHECK(hipMalloc((void**)&dZ, vecBytes));
    CHECK(hipMalloc((void**)&dDinv, vecBytes));
    CHECK(hipMemcpy(dV, hv, (size_t)hackSize * height * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dI, hi, (size_t)hackSize * height * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dHo, ho, hacks * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dRs, rowLen, (size_t)n * sizeof(int), hipMemcpyHostToDevice));

    /* b = A * ones is known only through r0 = b - A*0 = b: start from x = 0, exact solution = ones */
    double* b = (double*)calloc(n, sizeof(double));
    for (int e = 0; e < nnz; ++e)
        b[cr[e]] += cv[e];

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS) return 2;
    hipStream_t stream = spgpuGetStream(h);
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));
    printf("Jacobi-PCG on A = S L S, L the %d x %d 5-point Laplacian (%d rows, %d nnz), HELL hackSize %d, s_i in [10^-1.5, 10^1.5)\n",
           g, g, n, nnz, hackSize);

    /* ---- the preconditioner: the inverted diagonal, from the matrix as the library holds it ---- */
    spgpuDhellDiag(h, dDinv, dV, dI, hackSize, dHo, dRs, n, 0, 1);
    double* dinv = (double*)malloc(vecBytes);
    CHECK(hipMemcpy(dinv, dDinv, vecBytes, hipMemcpyDeviceToHost));
    int dinvWrong = 0;
    for (int i = 0; i < n; ++i) {
        const double want = 1.0 / ((scale[i] * 4.0) * scale[i]);
        dinvWrong += memcmp(&want, &dinv[i], sizeof(double)) != 0;
    }
    printf("dinv from spgpuDhellDiag: %s the host's 1 / (4 s_i^2) (%d of %d differ)\n", dinvWrong ? "DIFFERS from" : "equal to",
           dinvWrong, n);

    /* ---- (a) eager, host scalars ---- */
    CHECK(hipMemcpy(dR, b, vecBytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(dX, 0, vecBytes));
    spgpuDaxy(h, dZ, n, 1.0, dDinv, dR);                                                         /* z = M^-1 r      */
    CHECK(hipMemcpyAsync(dP, dZ, vecBytes, hipMemcpyDeviceToDevice, stream));                    /* p = z           */
    double rz = spgpuDdot(h, n, dR, dZ);
    double rr = spgpuDdot(h, n, dR, dR);
    const double rr0 = rr;
    printf("iter 0  |r| = %.6e\n", sqrt(rr));
    CHECK(hipEventRecord(t0, stream));
    int it = 0;
    while (it < maxIter && sqrt(rr / rr0) > tol) {
        spgpuDhellspmv(h, dAp, dAp, 1.0, dV, dI, hackSize, dHo, dRs, NULL, maxRow, n, dP, 0.0, 0); /* Ap = A p        */
        const double pAp = spgpuDdot(h, n, dP, dAp);
        const double alpha = rz / pAp;
        spgpuDaxpby(h, dX, n, 1.0, dX, alpha, dP);                                               /* x += alpha p    */
        spgpuDaxpby(h, dR, n, 1.0, dR, -alpha, dAp);                                             /* r -= alpha Ap   */
        spgpuDaxy(h, dZ, n, 1.0, dDinv, dR);                                                     /* z = M^-1 r      */
        const double rzNew = spgpuDdot(h, n, dR, dZ);
        rr = spgpuDdot(h, n, dR, dR);
        spgpuDaxpby(h, dP, n, rzNew / rz, dP, 1.0, dZ);                                          /* p = z + beta p  */
        rz = rzNew;
        ++it;
        if (it % 25 == 0 || sqrt(rr / rr0) <= tol)
            printf("iter %d  |r| = %.6e\n", it, sqrt(rr));
    }
    CHECK(hipEventRecord(t1, stream));
    CHECK(hipEventSynchronize(t1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, t0, t1));
    const int converged = sqrt(rr / rr0) <= tol;
    double* x = (double*)malloc(vecBytes);
    CHECK(hipMemcpy(x, dX, vecBytes, hipMemcpyDeviceToHost));
    double err = 0;
    for (int i = 0; i < n; ++i)
        if (fabs(x[i] - 1.0) > err)
            err = fabs(x[i] - 1.0);
    printf("PCG: %d iterations, %.3f ms total, %.1f us per iteration, relative residual %.3e (%s), max |x - 1| = %.3e\n", it, ms,
           it ? ms * 1e3 / it : 0.0, sqrt(rr / rr0), converged ? "converged" : "NOT converged", err);

    /* ---- (b) one captured graph per iteration, scalars on the device ---- */
    enum { RZ_A, RR_A, RZ_B, RR_B, PAP, SCALARS }; /* (r.z, |r|^2) alternates between two pairs of cells: no copy, no pointer swap */
    double* dS;
    CHECK(hipMalloc((void**)&dS, SCALARS * sizeof(double)));
    CHECK(hipMemcpy(dR, b, vecBytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(dX, 0, vecBytes));
    spgpuDaxyDotDevice(h, dS + RZ_A, n, dZ, dDinv, dR);                                          /* z = M^-1 r, r.z */
    CHECK(hipMemcpyAsync(dP, dZ, vecBytes, hipMemcpyDeviceToDevice, stream));
    hipGraph_t graph[2];
    hipGraphExec_t step[2];
    for (int parity = 0; parity < 2; ++parity) {
        double* cellsOld = dS + (parity ? RZ_B : RZ_A);
        double* cellsNew = dS + (parity ? RZ_A : RZ_B);
        CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeGlobal));
        spgpuDhellspmvDotDevice(h, dS + PAP, NULL, dAp, NULL, 1.0, dV, dI, hackSize, dHo, dRs, n, dP, 0.0, 0);
        spgpuDaxpbyPairAxyDotDevice(h, cellsNew, n, dX, dX, dP, dR, dR, dAp, dZ, dDinv, cellsOld, dS + PAP);
        spgpuDaxpbyQuotDevice(h, dP, n, cellsNew, cellsOld, dP, NULL, NULL, 0, dZ);
        CHECK(hipStreamEndCapture(stream, &graph[parity]));
        CHECK(hipGraphInstantiate(&step[parity], graph[parity], NULL, NULL, 0));
    }
    CHECK(hipEventRecord(t0, stream));
    for (int i = 0; i < it; ++i)
        CHECK(hipGraphLaunch(step[i & 1], stream));
    CHECK(hipEventRecord(t1, stream));
    CHECK(hipEventSynchronize(t1));
    float msGraph = 0;
    CHECK(hipEventElapsedTime(&msGraph, t0, t1));
    double* xg = (double*)malloc(vecBytes);
    double last[2] = {0, 0};
    CHECK(hipMemcpy(xg, dX, vecBytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(last, dS + ((it & 1) ? RZ_B : RZ_A), sizeof(last), hipMemcpyDeviceToHost));
    const int sameX = memcmp(x, xg, vecBytes) == 0;
    const int sameRz = memcmp(&rz, &last[0], sizeof(double)) == 0;
    const int sameRr = it == 0 || memcmp(&rr, &last[1], sizeof(double)) == 0; /* no iteration: the |r|^2 cell was never written */
    const int same = sameX && sameRz && sameRr;
    printf("graph replay: %d iterations, %.3f ms total, %.1f us per iteration (5 kernels; eager with host scalars: %.1f us); "
           "x %s, r.z %s, |r|^2 %s: %s\n", it, msGraph, it ? msGraph * 1e3 / it : 0.0, it ? ms * 1e3 / it : 0.0,
           sameX ? "same" : "DIFFERS", sameRz ? "same" : "DIFFERS", sameRr ? "same" : "DIFFERS",
           same ? "bit-identical to the eager run" : "DIFFERS from the eager run");
    for (int parity = 0; parity < 2; ++parity) {
        CHECK(hipGraphExecDestroy(step[parity]));
        CHECK(hipGraphDestroy(graph[parity]));
    }

    /* ---- (c) plain CG on the same matrix, eager, maxIter iterations ---- */
    CHECK(hipMemcpy(dR, b, vecBytes, hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dP, b, vecBytes, hipMemcpyHostToDevice));
    CHECK(hipMemset(dX, 0, vecBytes));
    double cr2 = spgpuDdot(h, n, dR, dR), crBest = cr2;
    int cgIt = 0;
    while (cgIt < maxIter && sqrt(cr2 / rr0) > tol) {
        spgpuDhellspmv(h, dAp, dAp, 1.0, dV, dI, hackSize, dHo, dRs, NULL, maxRow, n, dP, 0.0, 0);
        const double alpha = cr2 / spgpuDdot(h, n, dP, dAp);
        spgpuDaxpby(h, dX, n, 1.0, dX, alpha, dP);
        spgpuDaxpby(h, dR, n, 1.0, dR, -alpha, dAp);
        const double next = spgpuDdot(h, n, dR, dR);
        spgpuDaxpby(h, dP, n, next / cr2, dP, 1.0, dR);
        cr2 = next;
        crBest = cr2 < crBest ? cr2 : crBest;
        ++cgIt;
    }
    printf("plain CG: relative residual %.3e after %d iterations (smallest on the way %.3e)\n", sqrt(cr2 / rr0), cgIt,
           sqrt(crBest / rr0));

    spgpuDestroy(h);
    CHECK(hipGetLastError());
    const int ok = converged && same && dinvWrong == 0;
    printf(ok ? "PASSED\n" : "FAILED (PCG did not reach the tolerance, the graph run differs, or dinv is not the host's)\n");
    return ok ? 0 : 1;
}

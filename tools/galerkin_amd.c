/*
 * The Galerkin coarse operator A_c = P^T * A * P of a two-grid method, built on the device (spgpu/ext/spgemm_device.h), written
 * against the C ABI only.  A is the 5-point Laplacian on an n x n grid (4 on the diagonal, -1 to each neighbour inside the grid),
 * listed as COO contributions with the diagonal split in two and assembled (spgpu/ext/assemble_device.h); P aggregates 2 x 2 cells
 * with unit entries (n even, (n/2)^2 aggregates).  Base 1 everywhere.
 *   1. P goes into HELL (spgpu/ext/csr_device.h), P^T comes out of spgpuHellTransposeDevice and back to CSR through
 *      spgpuHellToCsrDevice; R = P^T * A and A_c = R * P are formed by spgpuCsrSpgemmProductsDevice / PlanDevice / Device; A_c goes
 *      into HELL and is multiplied once;
 *   2. A gets new coefficients (6 on the diagonal) through spgpuCooAssembleValuesDevice, and R, A_c and the HELL values follow
 *      through spgpuCsrSpgemmValuesDevice (twice) and spgpuCsrToHellValuesDevice; the matrix is multiplied again.
 * The closed form: A_c is again a 5-point stencil on the (n/2) x (n/2) grid, 4 d - 8 on the diagonal for a fine diagonal d and -2
 * to each neighbouring aggregate.  Every number is a small integer, so every sum is exact in fp64 and the comparisons are ==.
 *
 *   usage: galerkin_amd [n=64]
 * Prints the sizes, "<stage>: sum(z) sum((i % 7 + 1) * z[i]) sum(values of A_c)" for both stages and PASSED, or the first mismatch.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/convert_device.h"
#include "spgpu/hell.h"
#include "spgpu/ext/assemble_device.h"
#include "spgpu/ext/csr_device.h"
#include "spgpu/ext/spgemm_device.h"
#include "spgpu/ext/to_csr_device.h"
#include "spgpu/ext/transpose_device.h"
#include "spgpu/ext/update_device.h"

#define CHECK(call)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)

#define OK(call)                                                                          \
    do {                                                                                  \
        spgpuStatus_t s_ = (call);                                                        \
        if (s_ != SPGPU_SUCCESS) {                                                        \
            fprintf(stderr, "%s:%d: %s -> status %d\n", __FILE__, __LINE__, #call, s_);   \
            exit(2);                                                                      \
        }                                                                                 \
    } while (0)

enum { HACK = 32, BASE = 1 };

static void* deviceAlloc(size_t bytes)
{
    void* p;
    CHECK(hipMalloc(&p, bytes ? bytes : 16));
    return p;
}

static void* deviceCopyOf(const void* host, size_t bytes)
{
    void* p = deviceAlloc(bytes);
    CHECK(hipMemcpy(p, host, bytes, hipMemcpyHostToDevice));
    return p;
}

typedef struct Csr {
    int rows, cols, nnz;
    int* ptr;
    int* idx;
    double* val;
} Csr;

typedef struct Hell {
    double* cM;
    int* rP;
    int* hackOffsets;
    int* rS;
    int slots, longest;
} Hell;

/* the HELL arrays of a CSR matrix */
static void hellOf(spgpuHandle_t h, Hell* m, const Csr* a, void* planWork)
{
    int height = 0;
    m->rS = (int*)deviceAlloc((size_t)a->rows * sizeof(int));
    OK(spgpuCsrRowLengthsDevice(h, m->rS, &m->longest, a->rows, a->ptr, BASE));
    m->hackOffsets = (int*)deviceAlloc((size_t)((a->rows + HACK - 1) / HACK) * sizeof(int));
    OK(spgpuHellPlanDevice(h, &height, m->hackOffsets, HACK, a->rows, m->rS, planWork));
    m->slots = HACK * height;
    m->cM = (double*)deviceAlloc((size_t)m->slots * sizeof(double));
    m->rP = (int*)deviceAlloc((size_t)m->slots * sizeof(int));
    CHECK(hipMemset(m->cM, 0, (size_t)m->slots * sizeof(double)));
    CHECK(hipMemset(m->rP, 0, (size_t)m->slots * sizeof(int)));
    OK(spgpuCsrToHellDevice(h, m->cM, m->rP, m->hackOffsets, HACK, BASE, a->rows, a->ptr, a->idx, a->val, BASE, SPGPU_TYPE_DOUBLE, NULL));
}

/* C = A * B: the analysis and the first fill; the scratch is freed when the fill has passed on the stream */
static void multiply(spgpuHandle_t h, Csr* c, const Csr* a, const Csr* b, int* productsOut)
{
    int products = 0;
    void* small = deviceAlloc(spgpuCsrSpgemmWorkBytes(a->rows, b->cols, 0));
    OK(spgpuCsrSpgemmProductsDevice(h, &products, a->rows, a->cols, a->ptr, a->idx, b->ptr, BASE, small));
    CHECK(hipFree(small));
    void* work = deviceAlloc(spgpuCsrSpgemmWorkBytes(a->rows, b->cols, products));
    c->rows = a->rows, c->cols = b->cols;
    c->ptr = (int*)deviceAlloc(((size_t)a->rows + 1) * sizeof(int));
    OK(spgpuCsrSpgemmPlanDevice(h, &c->nnz, c->ptr, a->rows, a->cols, b->cols, a->ptr, a->idx, b->ptr, b->idx, BASE, products, work));
    c->idx = (int*)deviceAlloc((size_t)c->nnz * sizeof(int));
    c->val = (double*)deviceAlloc((size_t)c->nnz * sizeof(double));
    OK(spgpuCsrSpgemmDevice(h, c->idx, c->val, c->nnz, a->rows, a->ptr, a->idx, a->val, b->ptr, b->idx, b->val, c->ptr, BASE, SPGPU_TYPE_DOUBLE,
                            work));
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));
    CHECK(hipFree(work));
    *productsOut = products;
}

static void remultiply(spgpuHandle_t h, const Csr* c, const Csr* a, const Csr* b)
{
    OK(spgpuCsrSpgemmValuesDevice(h, c->val, a->rows, a->ptr, a->idx, a->val, b->ptr, b->idx, b->val, c->ptr, c->idx, BASE, SPGPU_TYPE_DOUBLE));
}

/* the closed form of A_c on the m x m coarse grid: the value at (I, J), 0 where the stencil has nothing */
static double coarseValue(int m, int I, int J, double fineDiagonal)
{
    const int xi = I % m, yi = I / m, xj = J % m, yj = J / m;
    const int dx = xi > xj ? xi - xj : xj - xi, dy = yi > yj ? yi - yj : yj - yi;
    if (dx + dy == 0)
        return 4.0 * fineDiagonal - 8.0;
    return dx + dy == 1 ? -2.0 : 0.0;
}

int main(int argc, char** argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 64;
    if (n < 2 || n > 4000 || n % 2) {
        fprintf(stderr, "usage: galerkin_amd [n: even, 2 .. 4000]\n");
        return 2;
    }
    const int m = n / 2, fine = n * n, coarse = m * m;

    /* ---- A as a list of contributions: the diagonal as 3 + 1 (then 5 + 1), each neighbour once ---- */
    int* ai = (int*)malloc((size_t)6 * fine * sizeof(int));
    int* aj = (int*)malloc((size_t)6 * fine * sizeof(int));
    double* v1 = (double*)malloc((size_t)6 * fine * sizeof(double));
    double* v2 = (double*)malloc((size_t)6 * fine * sizeof(double));
    int nnz = 0;
    for (int i = 0; i < fine; ++i) {
        const int x = i % n, y = i / n;
        const int to[4] = {x > 0 ? i - 1 : -1, x < n - 1 ? i + 1 : -1, y > 0 ? i - n : -1, y < n - 1 ? i + n : -1};
        for (int k = 0; k < 4; ++k)
            if (to[k] >= 0)
                ai[nnz] = i + BASE, aj[nnz] = to[k] + BASE, v1[nnz] = v2[nnz] = -1.0, ++nnz;
        ai[nnz] = i + BASE, aj[nnz] = i + BASE, v1[nnz] = 3.0, v2[nnz] = 5.0, ++nnz;
        ai[nnz] = i + BASE, aj[nnz] = i + BASE, v1[nnz] = 1.0, v2[nnz] = 1.0, ++nnz;
    }
    /* ---- P in CSR: fine cell (x, y) belongs to aggregate (x / 2, y / 2) ---- */
    int* pPtr = (int*)malloc(((size_t)fine + 1) * sizeof(int));
    int* pIdx = (int*)malloc((size_t)fine * sizeof(int));
    double* pVal = (double*)malloc((size_t)fine * sizeof(double));
    for (int i = 0; i < fine; ++i)
        pPtr[i] = i + BASE, pIdx[i] = (i / n / 2) * m + (i % n) / 2 + BASE, pVal[i] = 1.0;
    pPtr[fine] = fine + BASE;
    double* x = (double*)malloc((size_t)coarse * sizeof(double));
    for (int j = 0; j < coarse; ++j)
        x[j] = (double)(j % 13 + 1);

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS)
        return 2;
    int* dAi = (int*)deviceCopyOf(ai, (size_t)nnz * sizeof(int));
    int* dAj = (int*)deviceCopyOf(aj, (size_t)nnz * sizeof(int));
    double* dV1 = (double*)deviceCopyOf(v1, (size_t)nnz * sizeof(double));
    double* dV2 = (double*)deviceCopyOf(v2, (size_t)nnz * sizeof(double));
    double* dX = (double*)deviceCopyOf(x, (size_t)coarse * sizeof(double));
    double* z = (double*)deviceAlloc((size_t)coarse * sizeof(double));
    void* planWork = deviceAlloc(spgpuCooConvertWorkBytes(fine, 0));

    /* ---- A assembled ---- */
    Csr A = {fine, fine, 0, NULL, NULL, NULL};
    A.ptr = (int*)deviceAlloc(((size_t)fine + 1) * sizeof(int));
    int* perm = (int*)deviceAlloc((size_t)nnz * sizeof(int));
    int* segPtr = (int*)deviceAlloc(((size_t)nnz + 1) * sizeof(int));
    void* asmWork = deviceAlloc(spgpuCooAssembleWorkBytes(fine, fine, nnz));
    OK(spgpuCooAssemblePlanDevice(h, &A.nnz, A.ptr, perm, segPtr, fine, fine, nnz, dAi, dAj, BASE, BASE, asmWork));
    CHECK(hipFree(asmWork));
    A.idx = (int*)deviceAlloc((size_t)A.nnz * sizeof(int));
    A.val = (double*)deviceAlloc((size_t)A.nnz * sizeof(double));
    OK(spgpuCooAssembleDevice(h, A.idx, A.val, A.nnz, nnz, dAj, dV1, BASE, BASE, SPGPU_TYPE_DOUBLE, perm, segPtr));

    /* ---- P, and P^T through the transpose and back to CSR ---- */
    Csr P = {fine, coarse, fine, NULL, NULL, NULL};
    P.ptr = (int*)deviceCopyOf(pPtr, ((size_t)fine + 1) * sizeof(int));
    P.idx = (int*)deviceCopyOf(pIdx, (size_t)fine * sizeof(int));
    P.val = (double*)deviceCopyOf(pVal, (size_t)fine * sizeof(double));
    Hell hp, ht;
    hellOf(h, &hp, &P, planWork);
    void* tWork = deviceAlloc(spgpuHellTransposeWorkBytes(fine, coarse, hp.slots));
    int tNnz = 0, tHeight = 0;
    ht.rS = (int*)deviceAlloc((size_t)coarse * sizeof(int));
    OK(spgpuHellTransposeLengthsDevice(h, ht.rS, &ht.longest, &tNnz, hp.rP, HACK, hp.hackOffsets, hp.rS, NULL, fine, coarse, BASE, hp.slots, tWork));
    ht.hackOffsets = (int*)deviceAlloc((size_t)((coarse + HACK - 1) / HACK) * sizeof(int));
    OK(spgpuHellPlanDevice(h, &tHeight, ht.hackOffsets, HACK, coarse, ht.rS, tWork));
    ht.slots = HACK * tHeight;
    ht.cM = (double*)deviceAlloc((size_t)ht.slots * sizeof(double));
    ht.rP = (int*)deviceAlloc((size_t)ht.slots * sizeof(int));
    CHECK(hipMemset(ht.cM, 0, (size_t)ht.slots * sizeof(double)));
    CHECK(hipMemset(ht.rP, 0, (size_t)ht.slots * sizeof(int)));
    OK(spgpuHellTransposeDevice(h, ht.cM, ht.rP, ht.hackOffsets, HACK, BASE, hp.cM, hp.rP, HACK, hp.hackOffsets, hp.rS, NULL, fine, coarse, BASE,
                                hp.slots, SPGPU_TYPE_DOUBLE, ht.rS, tWork));
    Csr PT = {coarse, fine, 0, NULL, NULL, NULL};
    int ptLongest = 0;
    void* csrWork = deviceAlloc(spgpuToCsrWorkBytes(coarse));
    PT.ptr = (int*)deviceAlloc(((size_t)coarse + 1) * sizeof(int));
    OK(spgpuHellToCsrRowPtrDevice(h, PT.ptr, &PT.nnz, &ptLongest, BASE, HACK, ht.hackOffsets, ht.rS, NULL, coarse, ht.slots, csrWork));
    PT.idx = (int*)deviceAlloc((size_t)PT.nnz * sizeof(int));
    PT.val = (double*)deviceAlloc((size_t)PT.nnz * sizeof(double));
    OK(spgpuHellToCsrDevice(h, PT.idx, PT.val, PT.ptr, BASE, ht.cM, ht.rP, HACK, ht.hackOffsets, ht.rS, NULL, coarse, BASE, SPGPU_TYPE_DOUBLE));

    /* ---- R = P^T * A, A_c = R * P, A_c in HELL ---- */
    Csr R, Ac;
    int productsR = 0, productsC = 0;
    multiply(h, &R, &PT, &A, &productsR);
    multiply(h, &Ac, &R, &P, &productsC);
    Hell hc;
    hellOf(h, &hc, &Ac, planWork);
    printf("A: %d x %d, %d entries; P: %d aggregates; R = P^T A: %d products, %d entries; A_c = R P: %d products, %d entries, longest row %d\n",
           fine, fine, A.nnz, coarse, productsR, R.nnz, productsC, Ac.nnz, hc.longest);

    int* cPtr = (int*)malloc(((size_t)coarse + 1) * sizeof(int));
    int* cIdx = (int*)malloc((size_t)(Ac.nnz ? Ac.nnz : 1) * sizeof(int));
    double* cVal = (double*)malloc((size_t)(Ac.nnz ? Ac.nnz : 1) * sizeof(double));
    double* zh = (double*)malloc((size_t)coarse * sizeof(double));
    CHECK(hipMemcpy(cPtr, Ac.ptr, ((size_t)coarse + 1) * sizeof(int), hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(cIdx, Ac.idx, (size_t)Ac.nnz * sizeof(int), hipMemcpyDeviceToHost));
    int failed = 0;
    for (int stage = 0; stage < 2 && !failed; ++stage) {
        const char* name = stage ? "recomputed" : "built";
        const double fineDiagonal = stage ? 6.0 : 4.0;
        if (stage) { /* the step: new coefficients, every pattern as it was */
            OK(spgpuCooAssembleValuesDevice(h, A.val, A.nnz, nnz, dV2, SPGPU_TYPE_DOUBLE, perm, segPtr));
            remultiply(h, &R, &PT, &A);
            remultiply(h, &Ac, &R, &P);
            OK(spgpuCsrToHellValuesDevice(h, hc.cM, hc.hackOffsets, HACK, coarse, Ac.ptr, Ac.val, BASE, SPGPU_TYPE_DOUBLE, NULL));
        }
        spgpuDhellspmv(h, z, z, 1.0, hc.cM, hc.rP, HACK, hc.hackOffsets, hc.rS, NULL, 0, coarse, dX, 0.0, BASE);
        CHECK(hipStreamSynchronize(spgpuGetStream(h)));
        CHECK(hipMemcpy(zh, z, (size_t)coarse * sizeof(double), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(cVal, Ac.val, (size_t)Ac.nnz * sizeof(double), hipMemcpyDeviceToHost));
        double plain = 0.0, weighted = 0.0, stored = 0.0;
        for (int I = 0; I < coarse && !failed; ++I) {
            /* the row of A_c: exactly the stencil's entries, ascending, with the closed form's values */
            const int xi = I % m, yi = I / m;
            const int want[5] = {yi > 0 ? I - m : -1, xi > 0 ? I - 1 : -1, I, xi < m - 1 ? I + 1 : -1, yi < m - 1 ? I + m : -1};
            int at = cPtr[I] - BASE;
            double row = 0.0;
            for (int k = 0; k < 5; ++k) {
                if (want[k] < 0)
                    continue;
                const double value = coarseValue(m, I, want[k], fineDiagonal);
                if (at >= cPtr[I + 1] - BASE || cIdx[at] - BASE != want[k] || cVal[at] != value) {
                    printf("%s: row %d of A_c: entry (%d, %d) = %.17g expected at position %d\n", name, I, I, want[k], value, at);
                    failed = 1;
                    break;
                }
                row += value * x[want[k]];
                ++at;
            }
            if (!failed && at != cPtr[I + 1] - BASE) {
                printf("%s: row %d of A_c has %d entries too many\n", name, I, cPtr[I + 1] - BASE - at);
                failed = 1;
            }
            if (!failed && zh[I] != row) {
                printf("%s: z[%d] = %.17g, the closed form gives %.17g\n", name, I, zh[I], row);
                failed = 1;
            }
            plain += zh[I], weighted += (double)(I % 7 + 1) * zh[I];
        }
        for (int u = 0; u < Ac.nnz; ++u)
            stored += cVal[u];
        printf("%s: %.17g %.17g %.17g\n", name, plain, weighted, stored);
    }
    printf(failed ? "FAILED\n" : "PASSED\n");
    spgpuDestroy(h);
    CHECK(hipGetLastError());
    return failed;
}

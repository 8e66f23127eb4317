/*
 * The system matrix M + dt * K of an implicit time step, formed on the device (spgpu/ext/add_device.h), written against the C ABI
 * only.  K is the 5-point Laplacian on an n x n grid (4 on the diagonal, -1 to each neighbour inside the grid), M a narrower mass
 * matrix on the tridiagonal-in-x subset of that pattern (4 on the diagonal, 1 to the left and right neighbour).  Each is listed as
 * COO contributions with the diagonal split in two and assembled separately (spgpu/ext/assemble_device.h).  Base 1 everywhere.
 *   1. C = M + dt * K with dt = 1/2: spgpuCsrAddPlanDevice, spgpuCsrAddDevice; C goes into HELL (spgpu/ext/csr_device.h) and is
 *      multiplied by the vector of ones;
 *   2. K gets new coefficients (6 on the diagonal) through spgpuCooAssembleValuesDevice and dt becomes 1/4; C and the HELL values
 *      follow through spgpuCsrAddValuesDevice and spgpuCsrToHellValuesDevice; the matrix is multiplied again.
 * The closed form: row (x, y) of (M + dt * K) * 1 is 4 + mx + dt * (d - kx), with mx the number of x-neighbours inside the grid, kx
 * the number of all neighbours inside it and d the diagonal of K.  Every number is a small multiple of 1/4, so every sum is exact
 * in fp64 and the comparisons are ==.  M's pattern lies inside K's, so C has K's pattern.
 *
 *   usage: timestep_amd [n=64]
 * Prints the sizes, "<stage>: sum(z) sum((i % 7 + 1) * z[i]) sum(values of C)" for both stages and PASSED, or the first mismatch.
 * Exit status 0 only if both stages hold.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/convert_device.h"
#include "spgpu/hell.h"
#include "spgpu/ext/add_device.h"
#include "spgpu/ext/assemble_device.h"
#include "spgpu/ext/csr_device.h"
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
    int rows, nnz;
    int* ptr;
    int* idx;
    double* val;
} Csr;

/* a COO list in HBM with its assembly: perm and segPtr stay for the values-only pass */
typedef struct Listing {
    int nnz;
    int* cols;
    double* vals;
    int* perm;
    int* segPtr;
} Listing;

static void assemble(spgpuHandle_t h, Csr* m, Listing* l, int rows, const int* ai, const int* aj, const double* v, int nnz)
{
    int* dAi = (int*)deviceCopyOf(ai, (size_t)nnz * sizeof(int));
    l->nnz = nnz;
    l->cols = (int*)deviceCopyOf(aj, (size_t)nnz * sizeof(int));
    l->vals = (double*)deviceCopyOf(v, (size_t)nnz * sizeof(double));
    l->perm = (int*)deviceAlloc((size_t)nnz * sizeof(int));
    l->segPtr = (int*)deviceAlloc(((size_t)nnz + 1) * sizeof(int));
    m->rows = rows;
    m->ptr = (int*)deviceAlloc(((size_t)rows + 1) * sizeof(int));
    void* work = deviceAlloc(spgpuCooAssembleWorkBytes(rows, rows, nnz));
    OK(spgpuCooAssemblePlanDevice(h, &m->nnz, m->ptr, l->perm, l->segPtr, rows, rows, nnz, dAi, l->cols, BASE, BASE, work));
    CHECK(hipFree(work));
    CHECK(hipFree(dAi));
    m->idx = (int*)deviceAlloc((size_t)m->nnz * sizeof(int));
    m->val = (double*)deviceAlloc((size_t)m->nnz * sizeof(double));
    OK(spgpuCooAssembleDevice(h, m->idx, m->val, m->nnz, nnz, l->cols, l->vals, BASE, BASE, SPGPU_TYPE_DOUBLE, l->perm, l->segPtr));
}

int main(int argc, char** argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 64;
    if (n < 2 || n > 4000) {
        fprintf(stderr, "usage: timestep_amd [n: 2 .. 4000]\n");
        return 2;
    }
    const int rows = n * n;

    /* ---- K and M as lists of contributions: each diagonal in two parts, each neighbour once ---- */
    int* ki = (int*)malloc((size_t)6 * rows * sizeof(int));
    int* kj = (int*)malloc((size_t)6 * rows * sizeof(int));
    double* kv1 = (double*)malloc((size_t)6 * rows * sizeof(double));
    double* kv2 = (double*)malloc((size_t)6 * rows * sizeof(double));
    int* mi = (int*)malloc((size_t)4 * rows * sizeof(int));
    int* mj = (int*)malloc((size_t)4 * rows * sizeof(int));
    double* mv = (double*)malloc((size_t)4 * rows * sizeof(double));
    int kNnz = 0, mNnz = 0;
    for (int i = 0; i < rows; ++i) {
        const int x = i % n, y = i / n;
        const int to[4] = {x > 0 ? i - 1 : -1, x < n - 1 ? i + 1 : -1, y > 0 ? i - n : -1, y < n - 1 ? i + n : -1};
        for (int k = 0; k < 4; ++k)
            if (to[k] >= 0)
                ki[kNnz] = i + BASE, kj[kNnz] = to[k] + BASE, kv1[kNnz] = kv2[kNnz] = -1.0, ++kNnz;
        ki[kNnz] = i + BASE, kj[kNnz] = i + BASE, kv1[kNnz] = 3.0, kv2[kNnz] = 5.0, ++kNnz;
        ki[kNnz] = i + BASE, kj[kNnz] = i + BASE, kv1[kNnz] = 1.0, kv2[kNnz] = 1.0, ++kNnz;
        for (int k = 0; k < 2; ++k)
            if (to[k] >= 0)
                mi[mNnz] = i + BASE, mj[mNnz] = to[k] + BASE, mv[mNnz] = 1.0, ++mNnz;
        mi[mNnz] = i + BASE, mj[mNnz] = i + BASE, mv[mNnz] = 1.0, ++mNnz;
        mi[mNnz] = i + BASE, mj[mNnz] = i + BASE, mv[mNnz] = 3.0, ++mNnz;
    }
    double* ones = (double*)malloc((size_t)rows * sizeof(double));
    for (int j = 0; j < rows; ++j)
        ones[j] = 1.0;

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS)
        return 2;
    Csr K, M, Cm;
    Listing kList, mList;
    assemble(h, &K, &kList, rows, ki, kj, kv1, kNnz);
    assemble(h, &M, &mList, rows, mi, mj, mv, mNnz);
    double* dKv2 = (double*)deviceCopyOf(kv2, (size_t)kNnz * sizeof(double));
    double* dX = (double*)deviceCopyOf(ones, (size_t)rows * sizeof(double));
    double* z = (double*)deviceAlloc((size_t)rows * sizeof(double));

    /* ---- C = M + dt * K: the plan, once, and the first fill ---- */
    const double one = 1.0;
    double dt = 0.5;
    void* addWork = deviceAlloc(spgpuCsrAddWorkBytes(rows));
    Cm.rows = rows;
    Cm.ptr = (int*)deviceAlloc(((size_t)rows + 1) * sizeof(int));
    OK(spgpuCsrAddPlanDevice(h, &Cm.nnz, Cm.ptr, rows, rows, M.ptr, M.idx, K.ptr, K.idx, BASE, addWork));
    CHECK(hipFree(addWork)); /* the plan has synchronised, and no fill reads the scratch */
    Cm.idx = (int*)deviceAlloc((size_t)Cm.nnz * sizeof(int));
    Cm.val = (double*)deviceAlloc((size_t)Cm.nnz * sizeof(double));
    OK(spgpuCsrAddDevice(h, Cm.idx, Cm.val, Cm.nnz, rows, &one, M.ptr, M.idx, M.val, &dt, K.ptr, K.idx, K.val, Cm.ptr, BASE, SPGPU_TYPE_DOUBLE));

    /* ---- C in HELL ---- */
    int longest = 0, height = 0;
    int* rS = (int*)deviceAlloc((size_t)rows * sizeof(int));
    OK(spgpuCsrRowLengthsDevice(h, rS, &longest, rows, Cm.ptr, BASE));
    int* hackOffsets = (int*)deviceAlloc((size_t)((rows + HACK - 1) / HACK) * sizeof(int));
    void* planWork = deviceAlloc(spgpuCooConvertWorkBytes(rows, 0));
    OK(spgpuHellPlanDevice(h, &height, hackOffsets, HACK, rows, rS, planWork));
    const int slots = HACK * height;
    double* cM = (double*)deviceAlloc((size_t)slots * sizeof(double));
    int* rP = (int*)deviceAlloc((size_t)slots * sizeof(int));
    CHECK(hipMemset(cM, 0, (size_t)slots * sizeof(double)));
    CHECK(hipMemset(rP, 0, (size_t)slots * sizeof(int)));
    OK(spgpuCsrToHellDevice(h, cM, rP, hackOffsets, HACK, BASE, rows, Cm.ptr, Cm.idx, Cm.val, BASE, SPGPU_TYPE_DOUBLE, NULL));
    printf("K: %d x %d, %d entries; M: %d entries; C = M + dt K: %d entries, longest row %d\n", rows, rows, K.nnz, M.nnz, Cm.nnz, longest);

    double* zh = (double*)malloc((size_t)rows * sizeof(double));
    double* cVal = (double*)malloc((size_t)(Cm.nnz ? Cm.nnz : 1) * sizeof(double));
    int failed = Cm.nnz != K.nnz;
    if (failed)
        printf("C has %d entries, K's pattern has %d\n", Cm.nnz, K.nnz);
    for (int stage = 0; stage < 2 && !failed; ++stage) {
        const char* name = stage ? "stepped" : "built";
        const double diagonal = stage ? 6.0 : 4.0;
        if (stage) { /* the step: new coefficients for K and a new dt, every pattern as it was */
            dt = 0.25;
            OK(spgpuCooAssembleValuesDevice(h, K.val, K.nnz, kNnz, dKv2, SPGPU_TYPE_DOUBLE, kList.perm, kList.segPtr));
            OK(spgpuCsrAddValuesDevice(h, Cm.val, rows, &one, M.ptr, M.idx, M.val, &dt, K.ptr, K.idx, K.val, Cm.ptr, BASE, SPGPU_TYPE_DOUBLE));
            OK(spgpuCsrToHellValuesDevice(h, cM, hackOffsets, HACK, rows, Cm.ptr, Cm.val, BASE, SPGPU_TYPE_DOUBLE, NULL));
        }
        spgpuDhellspmv(h, z, z, 1.0, cM, rP, HACK, hackOffsets, rS, NULL, 0, rows, dX, 0.0, BASE);
        CHECK(hipStreamSynchronize(spgpuGetStream(h)));
        CHECK(hipMemcpy(zh, z, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(cVal, Cm.val, (size_t)Cm.nnz * sizeof(double), hipMemcpyDeviceToHost));
        double plain = 0.0, weighted = 0.0, stored = 0.0;
        for (int i = 0; i < rows; ++i) {
            const int x = i % n, y = i / n;
            const int mx = (x > 0) + (x < n - 1), kx = mx + (y > 0) + (y < n - 1);
            const double want = 4.0 + mx + dt * (diagonal - kx);
            if (zh[i] != want) {
                printf("%s: z[%d] = %.17g, the closed form gives %.17g\n", name, i, zh[i], want);
                failed = 1;
                break;
            }
            plain += zh[i], weighted += (double)(i % 7 + 1) * zh[i];
        }
        for (int u = 0; u < Cm.nnz; ++u)
            stored += cVal[u];
        if (!failed && stored != plain) { /* the sum of all entries is the sum of the row sums */
            printf("%s: the entries of C add up to %.17g, the row sums to %.17g\n", name, stored, plain);
            failed = 1;
        }
        printf("%s: %.17g %.17g %.17g\n", name, plain, weighted, stored);
    }
    printf(failed ? "FAILED\n" : "PASSED\n");
    spgpuDestroy(h);
    CHECK(hipGetLastError());
    return failed;
}

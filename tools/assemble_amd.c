/*
 * Assembly on the device (spgpu/ext/assemble_device.h), written against the C ABI only: what a finite-element code does before it
 * solves.  The P1 Laplacian on the unit square, n x n cells of two right triangles each, (n + 1)^2 nodes, is listed element by
 * element: nine contributions per triangle, twice the element matrix [[2,-1,-1],[-1,1,0],[-1,0,1]] (right-angle vertex first),
 * base 1, so that an interior matrix entry is listed up to six times.  The list is
 *   1. assembled (spgpuCooAssemblePlanDevice, spgpuCooAssembleDevice), the CSR arrays go into HELL in HBM
 *      (spgpuCsrRowLengthsDevice, spgpuHellPlanDevice, spgpuCsrToHellDevice) and the matrix is multiplied;
 *   2. assembled again with every element's matrix scaled by (element % 5 + 1) -- a coefficient that varies from element to
 *      element -- through spgpuCooAssembleValuesDevice and spgpuCsrToHellValuesDevice, and multiplied again;
 *   3. built both times with every duplicate kept (spgpuCooRowLengthsDevice, spgpuHellPlanDevice, spgpuCooToHellDevice) and
 *      multiplied: the products must be the same numbers.
 * Every value and every x[j] is a small integer: all sums are exact in fp64 in any order, and the comparison is ==.
 *
 *   usage: assemble_amd [n=40]
 * Prints the sizes, "<stage>: sum(z) sum((i % 7 + 1) * z[i]) sum(csrValues)" for both stages and PASSED, or the first mismatch.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/convert_device.h"
#include "spgpu/hell.h"
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

typedef struct Hell {
    double* cM;
    int* rP;
    int* hackOffsets;
    int* rS;
    int slots;
} Hell;

/* row lengths in m->rS: the HELL arrays, zeroed */
static void hellAlloc(spgpuHandle_t h, Hell* m, int hackSize, int rows, void* planWork)
{
    int height = 0;
    m->hackOffsets = (int*)deviceAlloc((size_t)((rows + hackSize - 1) / hackSize) * sizeof(int));
    OK(spgpuHellPlanDevice(h, &height, m->hackOffsets, hackSize, rows, m->rS, planWork));
    m->slots = hackSize * height;
    m->cM = (double*)deviceAlloc((size_t)m->slots * sizeof(double));
    m->rP = (int*)deviceAlloc((size_t)m->slots * sizeof(int));
    CHECK(hipMemset(m->cM, 0, (size_t)m->slots * sizeof(double)));
    CHECK(hipMemset(m->rP, 0, (size_t)m->slots * sizeof(int)));
}

/* z = A x, brought back to the host */
static void multiply(spgpuHandle_t h, double* hostZ, double* z, const Hell* m, int hackSize, int rows, const double* x, int base)
{
    spgpuDhellspmv(h, z, z, 1.0, m->cM, m->rP, hackSize, m->hackOffsets, m->rS, NULL, 0, rows, x, 0.0, base);
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));
    CHECK(hipMemcpy(hostZ, z, (size_t)rows * sizeof(double), hipMemcpyDeviceToHost));
}

int main(int argc, char** argv)
{
    const int n = argc > 1 ? atoi(argv[1]) : 40;
    const int hackSize = 32, base = 1;
    if (n < 1 || n > 2000) {
        fprintf(stderr, "usage: assemble_amd [n]\n");
        return 2;
    }
    const int rows = (n + 1) * (n + 1), elements = 2 * n * n, nnz = 9 * elements;
    static const int local[3][3] = {{2, -1, -1}, {-1, 1, 0}, {-1, 0, 1}};

    int* ai = (int*)malloc((size_t)nnz * sizeof(int));
    int* aj = (int*)malloc((size_t)nnz * sizeof(int));
    double* v1 = (double*)malloc((size_t)nnz * sizeof(double));
    double* v2 = (double*)malloc((size_t)nnz * sizeof(double));
    int at = 0;
    for (int e = 0; e < elements; ++e) {
        const int cell = e / 2, i = cell % n, j = cell / n;
        int node[3];
        if (e % 2 == 0) /* right angle at (i, j) */
            node[0] = j * (n + 1) + i, node[1] = node[0] + 1, node[2] = node[0] + n + 1;
        else            /* right angle at (i + 1, j + 1) */
            node[0] = (j + 1) * (n + 1) + i + 1, node[1] = node[0] - 1, node[2] = node[0] - (n + 1);
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b, ++at) {
                ai[at] = node[a] + base, aj[at] = node[b] + base;
                v1[at] = (double)local[a][b];
                v2[at] = (double)(local[a][b] * (e % 5 + 1));
            }
    }
    double* x = (double*)malloc((size_t)rows * sizeof(double));
    for (int j = 0; j < rows; ++j)
        x[j] = (double)(j % 13 + 1);

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS)
        return 2;
    int* dAi = (int*)deviceCopyOf(ai, (size_t)nnz * sizeof(int));
    int* dAj = (int*)deviceCopyOf(aj, (size_t)nnz * sizeof(int));
    double* dV1 = (double*)deviceCopyOf(v1, (size_t)nnz * sizeof(double));
    double* dV2 = (double*)deviceCopyOf(v2, (size_t)nnz * sizeof(double));
    double* dX = (double*)deviceCopyOf(x, (size_t)rows * sizeof(double));
    double* z = (double*)deviceAlloc((size_t)rows * sizeof(double));
    void* planWork = deviceAlloc(spgpuCooConvertWorkBytes(rows, 0));

    /* ---- the assembled matrix ---- */
    int* rowPtr = (int*)deviceAlloc(((size_t)rows + 1) * sizeof(int));
    int* perm = (int*)deviceAlloc((size_t)nnz * sizeof(int));
    int* segPtr = (int*)deviceAlloc(((size_t)nnz + 1) * sizeof(int));
    void* work = deviceAlloc(spgpuCooAssembleWorkBytes(rows, rows, nnz));
    int unique = 0, longest = 0;
    OK(spgpuCooAssemblePlanDevice(h, &unique, rowPtr, perm, segPtr, rows, rows, nnz, dAi, dAj, base, base, work));
    CHECK(hipFree(work)); /* the plan arrays are self-contained */
    int* csrCols = (int*)deviceAlloc((size_t)unique * sizeof(int));
    double* csrVals = (double*)deviceAlloc((size_t)unique * sizeof(double));
    OK(spgpuCooAssembleDevice(h, csrCols, csrVals, unique, nnz, dAj, dV1, base, base, SPGPU_TYPE_DOUBLE, perm, segPtr));
    Hell assembled;
    assembled.rS = (int*)deviceAlloc((size_t)rows * sizeof(int));
    OK(spgpuCsrRowLengthsDevice(h, assembled.rS, &longest, rows, rowPtr, base));
    hellAlloc(h, &assembled, hackSize, rows, planWork);
    OK(spgpuCsrToHellDevice(h, assembled.cM, assembled.rP, assembled.hackOffsets, hackSize, base, rows, rowPtr, csrCols, csrVals, base,
                            SPGPU_TYPE_DOUBLE, NULL));

    /* ---- the same list with every duplicate kept ---- */
    Hell kept;
    int keptLongest = 0;
    void* cooWork = deviceAlloc(spgpuCooConvertWorkBytes(rows, nnz));
    kept.rS = (int*)deviceAlloc((size_t)rows * sizeof(int));
    OK(spgpuCooRowLengthsDevice(h, kept.rS, &keptLongest, rows, nnz, dAi, base, cooWork));
    hellAlloc(h, &kept, hackSize, rows, planWork);
    printf("A: %d x %d, %d contributions, %d entries, longest row %d (kept: %d), slots %d (kept: %d)\n", rows, rows, nnz, unique, longest,
           keptLongest, assembled.slots, kept.slots);

    double* za = (double*)malloc((size_t)rows * sizeof(double));
    double* zk = (double*)malloc((size_t)rows * sizeof(double));
    double* sums = (double*)malloc((size_t)(unique ? unique : 1) * sizeof(double));
    int failed = 0;
    for (int stage = 0; stage < 2 && !failed; ++stage) {
        const double* values = stage ? dV2 : dV1;
        if (stage) { /* the step: new element matrices, the pattern as it was */
            OK(spgpuCooAssembleValuesDevice(h, csrVals, unique, nnz, values, SPGPU_TYPE_DOUBLE, perm, segPtr));
            OK(spgpuCsrToHellValuesDevice(h, assembled.cM, assembled.hackOffsets, hackSize, rows, rowPtr, csrVals, base, SPGPU_TYPE_DOUBLE, NULL));
        }
        OK(spgpuCooToHellDevice(h, kept.cM, kept.rP, kept.hackOffsets, hackSize, base, rows, nnz, dAi, dAj, values, base, SPGPU_TYPE_DOUBLE,
                                kept.rS, cooWork));
        multiply(h, za, z, &assembled, hackSize, rows, dX, base);
        multiply(h, zk, z, &kept, hackSize, rows, dX, base);
        CHECK(hipMemcpy(sums, csrVals, (size_t)unique * sizeof(double), hipMemcpyDeviceToHost));
        double plain = 0.0, weighted = 0.0, stored = 0.0;
        for (int i = 0; i < rows; ++i) {
            if (za[i] != zk[i] && !failed) {
                printf("%s: z[%d] = %.17g assembled, %.17g with duplicates kept\n", stage ? "scaled" : "built", i, za[i], zk[i]);
                failed = 1;
            }
            plain += za[i], weighted += (double)(i % 7 + 1) * za[i];
        }
        for (int u = 0; u < unique; ++u)
            stored += sums[u];
        printf("%s: %.17g %.17g %.17g\n", stage ? "scaled" : "built", plain, weighted, stored);
    }
    printf(failed ? "FAILED\n" : "PASSED\n");
    spgpuDestroy(h);
    CHECK(hipGetLastError());
    return failed;
}

/*
 * The transpose of a HELL matrix built on the device (spgpu/ext/transpose_device.h), written against the C ABI only: how a
 * caller gets trans = 'T' without leaving the GPU.
 * A rectangular banded matrix A (rows x cols, `band` entries per row around the scaled diagonal) is built in HBM from COO with
 * spgpuCooToHellDevice; A^T is built from the stored HELL arrays; spgpuDhellspmv runs on both and w'(A x) is printed beside
 * (A^T w)' x -- two different summation orders, so the two numbers are printed, not compared.  Then A^T is transposed again:
 * the rows of A are column-sorted and free of duplicates, so the result must be A's arrays, byte for byte (memcmp).
 *
 *   usage: transpose_amd [rows=200000] [cols=150000] [band=9]
 * Exits non-zero if a call fails or the double transpose differs.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/convert_device.h"
#include "spgpu/ext/transpose_device.h"
#include "spgpu/hell.h"
#include "spgpu/vector.h"

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

typedef struct {
    int rows, cols, hackSize, hacks, slots, longest, nnz;
    double* cM;
    int *rP, *hackOffsets, *rS;
} Hell;

static void* deviceAlloc(size_t bytes)
{
    void* p;
    CHECK(hipMalloc(&p, bytes ? bytes : 16));
    return p;
}

/* A^T of `a` as a HELL matrix with the same hack size and base 0 */
static Hell transposeOf(spgpuHandle_t h, const Hell* a)
{
    Hell t;
    t.rows = a->cols, t.cols = a->rows, t.hackSize = a->hackSize;
    t.hacks = (t.rows + t.hackSize - 1) / t.hackSize;
    const size_t workBytes = spgpuHellTransposeWorkBytes(a->rows, a->cols, a->slots);
    if (!workBytes) {
        fprintf(stderr, "spgpuHellTransposeWorkBytes returned 0\n");
        exit(2);
    }
    void* work = deviceAlloc(workBytes);
    t.rS = (int*)deviceAlloc((size_t)t.rows * sizeof(int));
    t.hackOffsets = (int*)deviceAlloc((size_t)t.hacks * sizeof(int));
    OK(spgpuHellTransposeLengthsDevice(h, t.rS, &t.longest, &t.nnz, a->rP, a->hackSize, a->hackOffsets, a->rS, NULL, a->rows, a->cols,
                                       0, a->slots, work));
    int height = 0;
    OK(spgpuHellPlanDevice(h, &height, t.hackOffsets, t.hackSize, t.rows, t.rS, work));
    t.slots = t.hackSize * height;
    t.cM = (double*)deviceAlloc((size_t)t.slots * sizeof(double));
    t.rP = (int*)deviceAlloc((size_t)t.slots * sizeof(int));
    CHECK(hipMemset(t.cM, 0, (size_t)t.slots * sizeof(double)));
    CHECK(hipMemset(t.rP, 0, (size_t)t.slots * sizeof(int)));
    OK(spgpuHellTransposeDevice(h, t.cM, t.rP, t.hackOffsets, t.hackSize, 0, a->cM, a->rP, a->hackSize, a->hackOffsets, a->rS, NULL,
                                a->rows, a->cols, 0, a->slots, SPGPU_TYPE_DOUBLE, t.rS, work));
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));
    CHECK(hipFree(work));
    return t;
}

static int sameDeviceBytes(const void* a, const void* b, size_t bytes)
{
    void* ha = malloc(bytes ? bytes : 1);
    void* hb = malloc(bytes ? bytes : 1);
    CHECK(hipMemcpy(ha, a, bytes, hipMemcpyDeviceToHost));
    CHECK(hipMemcpy(hb, b, bytes, hipMemcpyDeviceToHost));
    const int same = memcmp(ha, hb, bytes) == 0;
    free(ha);
    free(hb);
    return same;
}

int main(int argc, char** argv)
{
    const int rows = argc > 1 ? atoi(argv[1]) : 200000;
    const int cols = argc > 2 ? atoi(argv[2]) : 150000;
    const int band = argc > 3 ? atoi(argv[3]) : 9;
    const int hackSize = 32;
    if (rows < 1 || cols < 1 || band < 1 || (long long)rows * band > 2000000000LL) {
        fprintf(stderr, "usage: transpose_amd [rows] [cols] [band]\n");
        return 2;
    }

    /* COO, row-major, columns ascending inside a row and no duplicates; small integer values */
    int nnz = 0;
    int* cr = (int*)malloc((size_t)rows * band * sizeof(int));
    int* cc = (int*)malloc((size_t)rows * band * sizeof(int));
    double* cv = (double*)malloc((size_t)rows * band * sizeof(double));
    for (int i = 0; i < rows; ++i) {
        const int centre = (int)((long long)i * cols / rows);
        for (int d = -(band / 2); d < band - band / 2; ++d) {
            const int j = centre + d;
            if (j < 0 || j >= cols)
                continue;
            cr[nnz] = i, cc[nnz] = j, cv[nnz++] = (double)((i * 7 + j * 3) % 11 - 5);
        }
    }

    spgpuHandle_t h;
    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS)
        return 2;

    /* A in HBM through the COO route */
    Hell A;
    A.rows = rows, A.cols = cols, A.hackSize = hackSize, A.hacks = (rows + hackSize - 1) / hackSize, A.nnz = nnz;
    int* dCr = (int*)deviceAlloc((size_t)nnz * sizeof(int));
    int* dCc = (int*)deviceAlloc((size_t)nnz * sizeof(int));
    double* dCv = (double*)deviceAlloc((size_t)nnz * sizeof(double));
    CHECK(hipMemcpy(dCr, cr, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dCc, cc, (size_t)nnz * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dCv, cv, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    void* work = deviceAlloc(spgpuCooConvertWorkBytes(rows, nnz));
    A.rS = (int*)deviceAlloc((size_t)rows * sizeof(int));
    A.hackOffsets = (int*)deviceAlloc((size_t)A.hacks * sizeof(int));
    OK(spgpuCooRowLengthsDevice(h, A.rS, &A.longest, rows, nnz, dCr, 0, work));
    int height = 0;
    OK(spgpuHellPlanDevice(h, &height, A.hackOffsets, hackSize, rows, A.rS, work));
    A.slots = hackSize * height;
    A.cM = (double*)deviceAlloc((size_t)A.slots * sizeof(double));
    A.rP = (int*)deviceAlloc((size_t)A.slots * sizeof(int));
    CHECK(hipMemset(A.cM, 0, (size_t)A.slots * sizeof(double)));
    CHECK(hipMemset(A.rP, 0, (size_t)A.slots * sizeof(int)));
    OK(spgpuCooToHellDevice(h, A.cM, A.rP, A.hackOffsets, hackSize, 0, rows, nnz, dCr, dCc, dCv, 0, SPGPU_TYPE_DOUBLE, A.rS, work));
    CHECK(hipStreamSynchronize(spgpuGetStream(h)));
    printf("A: %d x %d, %d entries, longest row %d, %d HELL slots (hackSize %d)\n", rows, cols, nnz, A.longest, A.slots, hackSize);

    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));
    CHECK(hipEventRecord(t0, spgpuGetStream(h)));
    Hell T = transposeOf(h, &A);
    CHECK(hipEventRecord(t1, spgpuGetStream(h)));
    CHECK(hipEventSynchronize(t1));
    float ms = 0;
    CHECK(hipEventElapsedTime(&ms, t0, t1));
    printf("A^T: %d x %d, %d entries, longest row %d, %d HELL slots; built in %.3f ms (allocations included)\n", T.rows, T.cols, T.nnz,
           T.longest, T.slots, ms);

    /* w'(A x) beside (A^T w)'x */
    double* x = (double*)malloc((size_t)cols * sizeof(double));
    double* w = (double*)malloc((size_t)rows * sizeof(double));
    for (int j = 0; j < cols; ++j)
        x[j] = 1.0 + (double)(j % 13) / 16.0;
    for (int i = 0; i < rows; ++i)
        w[i] = 0.5 - (double)(i % 7) / 8.0;
    double* dX = (double*)deviceAlloc((size_t)cols * sizeof(double));
    double* dW = (double*)deviceAlloc((size_t)rows * sizeof(double));
    double* dAx = (double*)deviceAlloc((size_t)rows * sizeof(double));
    double* dAtw = (double*)deviceAlloc((size_t)cols * sizeof(double));
    CHECK(hipMemcpy(dX, x, (size_t)cols * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dW, w, (size_t)rows * sizeof(double), hipMemcpyHostToDevice));
    spgpuDhellspmv(h, dAx, dAx, 1.0, A.cM, A.rP, hackSize, A.hackOffsets, A.rS, NULL, A.longest, rows, dX, 0.0, 0);
    spgpuDhellspmv(h, dAtw, dAtw, 1.0, T.cM, T.rP, hackSize, T.hackOffsets, T.rS, NULL, T.longest, cols, dW, 0.0, 0);
    const double wAx = spgpuDdot(h, rows, dW, dAx);
    const double Atwx = spgpuDdot(h, cols, dAtw, dX);
    printf("w'(A x)    = %.17g\n(A^T w)' x = %.17g\n", wAx, Atwx);

    /* (A^T)^T against A */
    Hell B = transposeOf(h, &T);
    const int identical = B.rows == A.rows && B.cols == A.cols && B.nnz == A.nnz && B.longest == A.longest && B.slots == A.slots &&
                          sameDeviceBytes(B.rS, A.rS, (size_t)rows * sizeof(int)) &&
                          sameDeviceBytes(B.hackOffsets, A.hackOffsets, (size_t)A.hacks * sizeof(int)) &&
                          sameDeviceBytes(B.rP, A.rP, (size_t)A.slots * sizeof(int)) &&
                          sameDeviceBytes(B.cM, A.cM, (size_t)A.slots * sizeof(double));
    printf("double transpose: rS, hackOffsets, rP and cM %s\n", identical ? "identical to A's (memcmp)" : "DIFFER from A's");

    spgpuDestroy(h);
    CHECK(hipGetLastError());
    const int ok = identical && T.nnz == nnz;
    printf(ok ? "PASSED\n" : "FAILED\n");
    return ok ? 0 : 1;
}

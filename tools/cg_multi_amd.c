/*
 * Conjugate gradient for `count` right-hand sides at once on the 5-point Laplacian in HDIA, written against the C ABI only:
 * the consumer of the multivector SpMM (spgpu/ext/hdia_spmm.h) and of the device-scalar Level-1 calls on pitch multivectors
 * (spgpu/ext/device_scalars_mv.h).  Vector j of X, R, P and Ap starts at base + j*pitch; the bases are 16-byte aligned, the
 * pitch is a multiple of 16 bytes and larger than n, and the elements between n and the pitch hold a NaN pattern that no call
 * may read or write.  b_j = A*v_j for `count` different known v_j; every column starts from x = 0.
 *
 * Three legs of `iters` fixed iterations each, every one replayed from captured graphs (no host round trip):
 *   (a) reference  each column alone: spgpuDhdiaspmv, 2 spgpuDdotDevice, 3 spgpuDaxpbyQuotDevice per iteration (tools/cg_amd.c);
 *   (b) multi      one graph per block iteration: spgpuDhdiaspmmMv, 2 spgpuDmdotDevice, 3 spgpuDmaxpbyQuotDevice;
 *   (c) fused      spgpuDhdiaspmmMv, spgpuDmdotDevice, spgpuDmaxpbyPairDotDevice, spgpuDmaxpbyQuotDevice.
 * HDIA because its SpMM is contracted bit-identical to the SpMV per vector.  Where the cap on workgroups per vector of the
 * multivector reductions does not bind (device_scalars_mv.h), the iterates X and the final |r_j|^2 of (b) and (c) must equal
 * those of (a) bit for bit; where it binds the tool says so and requires only that every column's |r|^2 fell.
 *
 *   usage: cg_multi_amd [grid=64] [iters=20] [count=8]
 * Prints us per block iteration of each leg and PASSED / FAILED; exits non-zero on failure.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "spgpu/core.h"
#include "spgpu/hdia.h"
#include "spgpu/hdia_conv.h"
#include "spgpu/device_scalars.h"
#include "spgpu/ext/hdia_spmm.h"
#include "spgpu/ext/device_scalars_mv.h"

#define CHECK(call)                                                                                 \
    do {                                                                                            \
        hipError_t e_ = (call);                                                                     \
        if (e_ != hipSuccess) {                                                                     \
            fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
            exit(2);                                                                                \
        }                                                                                           \
    } while (0)

enum { REFERENCE, MULTI, FUSED, LEGS };
static const char* const legName[LEGS] = {"reference", "multi", "fused"};
static const uint64_t gapBits = 0x7ff8dead0000beefull; /* a quiet NaN no arithmetic produces */

static spgpuHandle_t h;
static int n, count, pitch, hackSize = 32;
static double *dM, *dX, *dR, *dP, *dAp, *dS; /* dS: |r|^2 (two arrays of count cells, alternating), p.Ap */
static int *dOff, *dHo;

static double* rrCell(int parity) { return dS + (parity ? count : 0); }
static double* pApCell(void) { return dS + 2 * count; }

/* One iteration that reads |r|^2 from rrCell(parity) and leaves the new one in rrCell(!parity). */
static void iteration(int leg, int parity, int column)
{
    double *rrOld = rrCell(parity), *rrNew = rrCell(!parity), *pAp = pApCell();
    if (leg == REFERENCE) {
        const size_t at = (size_t)column * pitch;
        double *x = dX + at, *r = dR + at, *p = dP + at, *ap = dAp + at;
        rrOld += column, rrNew += column, pAp += column;
        spgpuDhdiaspmv(h, ap, ap, 1.0, dM, dOff, hackSize, dHo, n, n, p, 0.0);      /* Ap = A p           */
        spgpuDdotDevice(h, pAp, n, p, ap);
        spgpuDaxpbyQuotDevice(h, x, n, NULL, NULL, x, rrOld, pAp, 0, p);             /* x += (rr/pAp) p    */
        spgpuDaxpbyQuotDevice(h, r, n, NULL, NULL, r, rrOld, pAp, 1, ap);            /* r -= (rr/pAp) Ap   */
        spgpuDdotDevice(h, rrNew, n, r, r);
        spgpuDaxpbyQuotDevice(h, p, n, rrNew, rrOld, p, NULL, NULL, 0, r);           /* p = r + (rr'/rr) p */
        return;
    }
    spgpuDhdiaspmmMv(h, dAp, NULL, 1.0, dM, dOff, hackSize, dHo, n, n, dP, 0.0, count, pitch, pitch);
    spgpuDmdotDevice(h, pAp, n, dP, dAp, count, pitch);
    if (leg == MULTI) {
        spgpuDmaxpbyQuotDevice(h, dX, n, NULL, NULL, dX, rrOld, pAp, 0, dP, count, pitch);
        spgpuDmaxpbyQuotDevice(h, dR, n, NULL, NULL, dR, rrOld, pAp, 1, dAp, count, pitch);
        spgpuDmdotDevice(h, rrNew, n, dR, dR, count, pitch);
    } else
        spgpuDmaxpbyPairDotDevice(h, rrNew, n, dX, dX, dP, dR, dR, dAp, rrOld, pAp, count, pitch);
    spgpuDmaxpbyQuotDevice(h, dP, n, rrNew, rrOld, dP, NULL, NULL, 0, dR, count, pitch);
}

static int gapsUntouched(const char* name, const double* device, double* scratch)
{
    CHECK(hipMemcpy(scratch, device, (size_t)pitch * count * sizeof(double), hipMemcpyDeviceToHost));
    for (int j = 0; j < count; ++j)
        for (int i = n; i < pitch; ++i)
            if (memcmp(scratch + (size_t)j * pitch + i, &gapBits, sizeof(double)) != 0) {
                printf("%s: element %d behind vector %d was written\n", name, i - n, j);
                return 0;
            }
    return 1;
}

int main(int argc, char** argv)
{
    const int g = argc > 1 ? atoi(argv[1]) : 64;
    const int iters = argc > 2 ? atoi(argv[2]) : 20;
    count = argc > 3 ? atoi(argv[3]) : 8;
    if (g < 2 || iters < 1 || count < 1) {
        fprintf(stderr, "usage: cg_multi_amd [grid=64] [iters=20] [count=8]\n");
        return 2;
    }
    n = g * g;
    pitch = (n + 2) & ~1; /* doubles: a multiple of 16 bytes, n + 1 or n + 2 */
    const size_t mvElems = (size_t)pitch * count, mvBytes = mvElems * sizeof(double);

    /* 5-point Laplacian in COO, natural order, then HDIA */
    int nnz = 0;
    int* cr = (int*)malloc((size_t)5 * n * sizeof(int));
    int* cc = (int*)malloc((size_t)5 * n * sizeof(int));
    double* cv = (double*)malloc((size_t)5 * n * sizeof(double));
    for (int i = 0; i < n; ++i) {
        const int gx = i % g, gy = i / g;
        if (gy > 0)     { cr[nnz] = i; cc[nnz] = i - g; cv[nnz++] = -1.0; }
        if (gx > 0)     { cr[nnz] = i; cc[nnz] = i - 1; cv[nnz++] = -1.0; }
        cr[nnz] = i; cc[nnz] = i; cv[nnz++] = 4.0;
        if (gx < g - 1) { cr[nnz] = i; cc[nnz] = i + 1; cv[nnz++] = -1.0; }
        if (gy < g - 1) { cr[nnz] = i; cc[nnz] = i + g; cv[nnz++] = -1.0; }
    }
    const int hacks = getHdiaHacksCount(hackSize, n);
    int height = 0;
    int* ho = (int*)calloc((size_t)hacks + 1, sizeof(int));
    computeHdiaHackOffsetsFromCoo(&height, ho, hackSize, n, n, nnz, cr, cc, 0);
    double* hv = (double*)calloc((size_t)hackSize * height, sizeof(double));
    int* hoff = (int*)calloc((size_t)height, sizeof(int));
    cooToHdia(hv, hoff, ho, hackSize, n, n, nnz, cr, cc, cv, 0, SPGPU_TYPE_DOUBLE);

    /* the start state as host images: vectors inside, the NaN pattern in every gap */
    double* v = (double*)malloc(mvBytes);     /* the known solutions */
    double* b = (double*)malloc(mvBytes);     /* R and P at the start */
    double* zero = (double*)malloc(mvBytes);  /* X at the start */
    double* blank = (double*)malloc(mvBytes); /* Ap at the start: nothing but the pattern */
    double* back = (double*)malloc(mvBytes);
    for (size_t e = 0; e < mvElems; ++e) {
        memcpy(v + e, &gapBits, sizeof(double));
        memcpy(b + e, &gapBits, sizeof(double));
        memcpy(zero + e, &gapBits, sizeof(double));
        memcpy(blank + e, &gapBits, sizeof(double));
    }
    for (int j = 0; j < count; ++j) {
        double *vj = v + (size_t)j * pitch, *bj = b + (size_t)j * pitch;
        for (int i = 0; i < n; ++i) {
            vj[i] = 1.0 + (double)(((long long)i * (j + 3) + 7 * j) % 17) / 8.0;
            bj[i] = 0.0;
            zero[(size_t)j * pitch + i] = 0.0;
        }
        for (int e = 0; e < nnz; ++e)
            bj[cr[e]] += cv[e] * vj[cc[e]];
    }

    CHECK(hipMalloc((void**)&dM, (size_t)hackSize * height * sizeof(double)));
    CHECK(hipMalloc((void**)&dOff, (size_t)height * sizeof(int)));
    CHECK(hipMalloc((void**)&dHo, ((size_t)hacks + 1) * sizeof(int)));
    CHECK(hipMalloc((void**)&dX, mvBytes));
    CHECK(hipMalloc((void**)&dR, mvBytes));
    CHECK(hipMalloc((void**)&dP, mvBytes));
    CHECK(hipMalloc((void**)&dAp, mvBytes));
    CHECK(hipMalloc((void**)&dS, (size_t)3 * count * sizeof(double)));
    CHECK(hipMemcpy(dM, hv, (size_t)hackSize * height * sizeof(double), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dOff, hoff, (size_t)height * sizeof(int), hipMemcpyHostToDevice));
    CHECK(hipMemcpy(dHo, ho, ((size_t)hacks + 1) * sizeof(int), hipMemcpyHostToDevice));

    if (spgpuCreate(&h, 0) != SPGPU_SUCCESS) return 2;
    hipStream_t stream = spgpuGetStream(h);
    hipEvent_t t0, t1;
    CHECK(hipEventCreate(&t0));
    CHECK(hipEventCreate(&t1));

    /* the condition under which the multivector reductions repeat the single-vector ones (device_scalars_mv.h) */
    const long long blocksAlone = ((n + 1) / 2 + 1023) / 1024;
    const int capFree = blocksAlone * count <= 1024;
    printf("block CG, %d right-hand sides on the %d x %d 5-point Laplacian (%d rows, %d nnz), HDIA hackSize %d, pitch %d\n", count,
           g, g, n, nnz, hackSize, pitch);
    printf("reductions: %lld workgroups per vector alone x %d vectors %s 1024: the cap %s\n", blocksAlone, count,
           capFree ? "<=" : ">", capFree ? "does not bind, bit identity with the per-column run is required" :
           "binds, bit identity with the per-column run is not contracted: only the fall of every |r|^2 is required");

    double* xOf[LEGS];
    double* rrOf[LEGS];
    double* rr0 = (double*)malloc(count * sizeof(double));
    float us[LEGS];
    int ok = 1;
    for (int leg = 0; leg < LEGS; ++leg) {
        const int graphs = leg == REFERENCE ? count : 1;
        hipGraph_t* graph = (hipGraph_t*)malloc((size_t)2 * graphs * sizeof(hipGraph_t));
        hipGraphExec_t* step = (hipGraphExec_t*)malloc((size_t)2 * graphs * sizeof(hipGraphExec_t));
        for (int pass = 0; pass < 2; ++pass) { /* pass 0: one eager iteration loads the kernels; pass 1: the start state for the run */
            CHECK(hipMemcpy(dX, zero, mvBytes, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(dR, b, mvBytes, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(dP, b, mvBytes, hipMemcpyHostToDevice));
            CHECK(hipMemcpy(dAp, blank, mvBytes, hipMemcpyHostToDevice));
            if (leg == REFERENCE)
                for (int j = 0; j < count; ++j)
                    spgpuDdotDevice(h, rrCell(0) + j, n, dR + (size_t)j * pitch, dR + (size_t)j * pitch);
            else
                spgpuDmdotDevice(h, rrCell(0), n, dR, dR, count, pitch);
            if (pass == 0)
                for (int j = 0; j < graphs; ++j)
                    iteration(leg, 0, j);
            CHECK(hipStreamSynchronize(stream));
        }
        CHECK(hipMemcpy(back, rrCell(0), count * sizeof(double), hipMemcpyDeviceToHost));
        if (leg == REFERENCE)
            memcpy(rr0, back, count * sizeof(double));
        else if (capFree && memcmp(rr0, back, count * sizeof(double)) != 0) {
            printf("%s: the initial |r|^2 DIFFERS from the per-column reference\n", legName[leg]);
            ok = 0;
        }
        for (int j = 0; j < graphs; ++j)
            for (int parity = 0; parity < 2; ++parity) {
                CHECK(hipStreamBeginCapture(stream, hipStreamCaptureModeGlobal));
                iteration(leg, parity, j);
                CHECK(hipStreamEndCapture(stream, &graph[2 * j + parity]));
                CHECK(hipGraphInstantiate(&step[2 * j + parity], graph[2 * j + parity], NULL, NULL, 0));
            }
        CHECK(hipEventRecord(t0, stream));
        for (int j = 0; j < graphs; ++j)
            for (int i = 0; i < iters; ++i)
                CHECK(hipGraphLaunch(step[2 * j + (i & 1)], stream));
        CHECK(hipEventRecord(t1, stream));
        CHECK(hipEventSynchronize(t1));
        float ms = 0;
        CHECK(hipEventElapsedTime(&ms, t0, t1));
        us[leg] = ms * 1e3f / iters;
        for (int k = 0; k < 2 * graphs; ++k) {
            CHECK(hipGraphExecDestroy(step[k]));
            CHECK(hipGraphDestroy(graph[k]));
        }
        free(graph);
        free(step);

        xOf[leg] = (double*)malloc(mvBytes);
        rrOf[leg] = (double*)malloc(count * sizeof(double));
        CHECK(hipMemcpy(xOf[leg], dX, mvBytes, hipMemcpyDeviceToHost));
        CHECK(hipMemcpy(rrOf[leg], rrCell(iters & 1), count * sizeof(double), hipMemcpyDeviceToHost));
        const int clean = gapsUntouched("X", dX, back) & gapsUntouched("R", dR, back) & gapsUntouched("P", dP, back) &
                          gapsUntouched("Ap", dAp, back);
        int fell = 1;
        double worst = 0, err = 0;
        for (int j = 0; j < count; ++j) {
            fell = fell && rrOf[leg][j] < rr0[j]; /* false for a NaN as well */
            if (!(sqrt(rrOf[leg][j] / rr0[j]) <= worst))
                worst = sqrt(rrOf[leg][j] / rr0[j]);
            for (int i = 0; i < n; ++i) {
                const double d = fabs(xOf[leg][(size_t)j * pitch + i] - v[(size_t)j * pitch + i]);
                if (!(d <= err))
                    err = d;
            }
        }
        printf("%-9s %d iterations, %.1f us per block iteration; largest relative residual %.3e, max |x_j - v_j| = %.3e; gaps %s\n",
               legName[leg], iters, us[leg], worst, err, clean ? "untouched" : "TOUCHED");
        ok = ok && clean && fell;
        if (!fell)
            printf("%s: the |r|^2 of a column did not fall\n", legName[leg]);
        if (leg != REFERENCE && capFree) {
            int same = memcmp(rrOf[leg], rrOf[REFERENCE], count * sizeof(double)) == 0;
            for (int j = 0; j < count; ++j)
                same = same && memcmp(xOf[leg] + (size_t)j * pitch, xOf[REFERENCE] + (size_t)j * pitch, (size_t)n * sizeof(double)) == 0;
            printf("%-9s iterates and |r|^2 of all %d columns %s\n", legName[leg], count,
                   same ? "bit-identical to the per-column reference" : "DIFFER from the per-column reference");
            ok = ok && same;
        }
    }
    printf("per block iteration: reference %.1f us, multi %.1f us (x%.2f), fused %.1f us (x%.2f)\n", us[REFERENCE], us[MULTI],
           us[REFERENCE] / us[MULTI], us[FUSED], us[REFERENCE] / us[FUSED]);

    spgpuDestroy(h);
    CHECK(hipGetLastError());
    printf(ok ? "PASSED\n" : "FAILED (a column's residual did not fall, a gap was touched, or a leg differs from the reference)\n");
    return ok ? 0 : 1;
}

/* vqa_demo.c — the C ABI of include/vqa.h from plain C (no Python, no torch): synthetic frames in pinned
 * memory, the full complexity suite and PSNR/SSIM, a few numbers printed.
 *   gcc -O2 -Iinclude -o vqa_demo examples/vqa_demo.c -Lreal-time-video-quality-analysis_amd/csrc -lvqa_hip \
 *       -Wl,-rpath,$PWD/real-time-video-quality-analysis_amd/csrc -lm
 * Exit code 0 = every call succeeded and the self-checks (Parseval, histogram mass, SSE of ref vs ref+1) hold. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "vqa.h"

#define CHECK(call)                                                                                   \
    do {                                                                                              \
        int rc_ = (call);                                                                             \
        if (rc_ != VQA_OK) {                                                                          \
            fprintf(stderr, "%s -> %s (%s)\n", #call, vqa_strerror(rc_), ctx ? vqa_last_hip_error(ctx) : ""); \
            return 2;                                                                                 \
        }                                                                                             \
    } while (0)

int main(void)
{
    vqa_ctx *ctx = NULL;
    const int n = 4, h = 270, w = 480;
    const size_t fb = (size_t)h * w * 3;
    if (vqa_abi_version() != VQA_ABI_VERSION) { fprintf(stderr, "ABI mismatch\n"); return 2; }
    CHECK(vqa_create(0, &ctx));
    uint8_t *ref = NULL, *dist = NULL;
    CHECK(vqa_alloc_pinned(ctx, fb * (n + 1), (void **)&ref));
    CHECK(vqa_alloc_pinned(ctx, fb * (n + 1), (void **)&dist));
    unsigned s = 12345u;
    for (size_t i = 0; i < fb * (n + 1); i++) { /* smooth-ish texture; dist = ref + 1 (clipped below 255) */
        s = s * 1664525u + 1013904223u;
        const unsigned v = ((i / 3 % w) * 3 + (i / (3 * w) % h) * 2 + (s >> 28)) & 0xff;
        ref[i] = (uint8_t)(v > 254 ? 254 : v);
        dist[i] = (uint8_t)(ref[i] + 1);
    }
    vqa_params p;
    vqa_default_params(&p);
    vqa_frame_metrics *fm = (vqa_frame_metrics *)calloc(n, sizeof *fm);
    CHECK(vqa_complexity_submit(ctx, dist + fb, dist, VQA_MEM_HOST, n, h, w, (int64_t)fb, (int64_t)w * 3, VQA_M_ALL, &p));
    vqa_plane_desc planes[3];
    for (int c = 0; c < 3; c++) {
        planes[c].width = w; planes[c].height = h; planes[c].offset = c; planes[c].row_stride = (int64_t)w * 3;
        planes[c].pixel_step = 3; planes[c].bit_depth = 0;
    }
    vqa_plane_metrics pm[4 * 3];
    CHECK(vqa_quality_submit(ctx, ref + fb, dist + fb, VQA_MEM_HOST, n, (int64_t)fb, (int64_t)fb, planes, 3, VQA_SSIM_GAUSS));
    CHECK(vqa_complexity_wait(ctx, fm, n));
    CHECK(vqa_quality_wait(ctx, pm, n * 3));
    int bad = 0;
    for (int i = 0; i < n; i++) {
        unsigned long long mass = 0;
        for (int b = 0; b < 256; b++) mass += fm[i].hist_gray[b];
        const double parseval = fabs(fm[i].dct_energy - (double)fm[i].sum_gray2) / (double)fm[i].sum_gray2;
        printf("frame %d: edges %u  dct_energy %.6g (Parseval rel.err %.1e)  sad/blk %.1f  orb %u  B-plane sse %llu ssim %.6f\n",
               i, fm[i].edge_count, fm[i].dct_energy, parseval,
               fm[i].sad_blocks ? (double)fm[i].sad_sum / fm[i].sad_blocks : 0.0, fm[i].orb_keypoints,
               (unsigned long long)pm[i * 3].sse, pm[i * 3].ssim);
        bad += mass != (unsigned long long)h * w;           /* every pixel lands in exactly one bin */
        bad += parseval > 1e-4;                              /* sum coef^2 == sum gray^2            */
        bad += pm[i * 3].sse != (unsigned long long)h * w;   /* ref vs ref + 1: SSE == pixel count  */
        bad += !(pm[i * 3].ssim > 0.99 && pm[i * 3].ssim < 1.0);
        bad += fm[i].has_prev != 1u;
    }
    /* VMAF's motion feature of the reference frames of the same pair sequence (frame 0 is the one before them) */
    {
        vqa_motion_metrics mm[4 * 3];
        CHECK(vqa_motion_submit(ctx, ref + fb, ref, VQA_MEM_HOST, n, (int64_t)fb, planes, 3));
        CHECK(vqa_motion_wait(ctx, mm, n * 3));
        for (int i = 0; i < n; i++) {
            printf("frame %d: B-plane motion %.6f (sad %.1f)\n", i, mm[i * 3].motion, mm[i * 3].sad);
            bad += !(mm[i * 3].motion > 0.0) || mm[i * 3].motion != mm[i * 3].sad / ((double)h * w);
        }
    }
    /* the path's one collective: pooled scalars summed over the communicator's devices (here: this one device,
     * so the sum is the input).  A multi-GPU host passes one ctx per device, or joins by rank (vqa_comm_create_rank). */
    {
        vqa_comm *comm = NULL;
        double pooled[2] = {fm[n - 1].dct_energy, (double)n};
        const double want0 = pooled[0];
        int rc = vqa_comm_create(&ctx, 1, &comm);
        if (rc == VQA_ERR_UNSUPPORTED) {
            puts("RCCL not installed: collective skipped");
        } else {
            if (rc != VQA_OK) { fprintf(stderr, "vqa_comm_create -> %s\n", vqa_strerror(rc)); return 2; }
            CHECK(vqa_allreduce(comm, pooled, 2));
            printf("all-reduce over %d device(s): dct_energy %.6g frames %.0f\n", vqa_comm_size(comm), pooled[0], pooled[1]);
            bad += pooled[0] != want0 || pooled[1] != (double)n;
            CHECK(vqa_comm_destroy(comm));
        }
    }
    free(fm);
    CHECK(vqa_free_pinned(ctx, ref));
    CHECK(vqa_free_pinned(ctx, dist));
    CHECK(vqa_destroy(ctx));
    if (bad) { fprintf(stderr, "%d self-checks failed\n", bad); return 1; }
    puts("vqa_demo ok");
    return 0;
}

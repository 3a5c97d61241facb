// render_bwd_args_check.cpp - the argument checks of the three backward launchers of mpf_render_bwd.hip as a stand-alone host program, for a
// sanitizer build that needs no GPU: every call below must be refused with MPF_ERR_BAD_ARGUMENT before anything is launched or dereferenced.
//
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -ffp-contract=off -fhip-fp32-correctly-rounded-divide-sqrt -Xarch_host -fsanitize=address,undefined \
//         tools/render_bwd_args_check.cpp mpiflow_amd/csrc/mpf_render_bwd.hip mpiflow_amd/csrc/mpf_generic.hip -o render_bwd_args_check
//   ./render_bwd_args_check          (prints "ok: N refusals", exit status 0)
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../include/mpiflow_hip.h"

static int g_failures = 0, g_checks = 0;

static void refused(int rc, const char *needle, const char *what)
{
    ++g_checks;
    const char *msg = mpf_last_error();
    if (rc != MPF_ERR_BAD_ARGUMENT || (needle && !strstr(msg, needle))) {
        fprintf(stderr, "NOT refused as expected: %s -> rc %d, message \"%s\"\n", what, rc, msg);
        ++g_failures;
    }
}

int main(void)
{
    float *const p = reinterpret_cast<float *>(uintptr_t(256));          // never dereferenced: a launcher that got this far has already failed the test
    float *const odd = reinterpret_cast<float *>(uintptr_t(260));
    const float *const n = nullptr;
    float *const nn = nullptr;
    const int64_t N = 16;

    refused(mpf_volume_render_bwd(n, n, n, n, 4, N, 0, 0, n, n, n, n, n, nn, nn, nn, nullptr), "null pointer", "volume: all null");
    refused(mpf_volume_render_bwd(n, p, p, n, 4, N, 0, 0, n, n, n, n, n, nn, nn, nn, nullptr), "null pointer", "volume: no grad_sigma");
    refused(mpf_volume_render_bwd(n, p, p, n, 0, N, 0, 0, n, n, n, n, n, nn, p, nn, nullptr), "bad shape", "volume: S = 0");
    refused(mpf_volume_render_bwd(n, p, p, n, 4096, N, 0, 0, n, n, n, n, n, nn, p, nn, nullptr), "bad shape", "volume: S = 4096");
    refused(mpf_volume_render_bwd(n, p, p, n, -3, N, 0, 0, n, n, n, n, n, nn, p, nn, nullptr), "bad shape", "volume: S < 0");
    refused(mpf_volume_render_bwd(n, p, p, n, 4, 0, 0, 0, n, n, n, n, n, nn, p, nn, nullptr), "bad shape", "volume: N = 0");
    refused(mpf_volume_render_bwd(n, p, p, n, 4, -(int64_t(1) << 40), 0, 0, n, n, n, n, n, nn, p, nn, nullptr), "bad shape", "volume: N < 0");
    refused(mpf_volume_render_bwd(n, p, p, p, 4, N, 5, 0, n, n, n, n, n, nn, p, nn, nullptr), "extra channels", "volume: E = 5");
    refused(mpf_volume_render_bwd(n, p, p, p, 4, N, -1, 0, n, n, n, n, n, nn, p, nn, nullptr), "extra channels", "volume: E < 0");
    refused(mpf_volume_render_bwd(n, p, p, n, 4, N, 2, 0, n, n, n, n, n, nn, p, nn, nullptr), "extra channels", "volume: E = 2 without extra_in");
    refused(mpf_volume_render_bwd(n, p, p, p, 4, N, 0, 0, n, n, n, n, n, nn, p, nn, nullptr), "extra channels", "volume: extra_in with E = 0");
    refused(mpf_volume_render_bwd(n, p, p, n, 4, N, 0, 0, n, n, p, n, n, nn, p, nn, nullptr), "extra gradients", "volume: g_extra with E = 0");
    refused(mpf_volume_render_bwd(n, p, p, n, 4, N, 0, 0, p, n, n, n, n, nn, p, nn, nullptr), "rgb gradients", "volume: g_rgb without rgb");
    refused(mpf_volume_render_bwd(n, p, p, n, 4, N, 0, 0, n, n, n, n, n, p, p, nn, nullptr), "rgb gradients", "volume: grad_rgb without rgb");
    refused(mpf_volume_render_bwd(p, p, p, p, 4, N, 2, 1, n, n, p, n, n, nn, p, p, nullptr), "hard", "volume: hard with rgb");
    refused(mpf_volume_render_bwd(n, p, p, p, 4, N, 2, 1, n, p, p, n, n, nn, p, p, nullptr), "hard", "volume: hard with g_depth");

    refused(mpf_homography_sample_bwd(n, n, 4, 3, 8, 8, 0, 3, nn, nullptr), "null pointer", "sample: all null");
    refused(mpf_homography_sample_bwd(p, p, 0, 3, 8, 8, 0, 3, p, nullptr), "bad shape", "sample: S = 0");
    refused(mpf_homography_sample_bwd(p, p, 65536, 3, 8, 8, 0, 3, p, nullptr), "bad shape", "sample: S = 65536");
    refused(mpf_homography_sample_bwd(p, p, 4, 0, 8, 8, 0, 3, p, nullptr), "bad shape", "sample: C = 0");
    refused(mpf_homography_sample_bwd(p, p, 4, 3, -8, 8, 0, 3, p, nullptr), "bad shape", "sample: H < 0");
    refused(mpf_homography_sample_bwd(p, p, 4, 3, 1 << 16, 1 << 16, 0, 3, p, nullptr), "too large", "sample: H*W = 2^32");
    refused(mpf_homography_sample_bwd(p, p, 4, 3, 8, 8, -1, 3, p, nullptr), "channel range", "sample: c0 < 0");
    refused(mpf_homography_sample_bwd(p, p, 4, 3, 8, 8, 2, 2, p, nullptr), "channel range", "sample: empty range");
    refused(mpf_homography_sample_bwd(p, p, 4, 3, 8, 8, 0, 4, p, nullptr), "channel range", "sample: c1 > C");
    refused(mpf_homography_sample_bwd(p, p, 4, 3, 8, 8, 3, 1, p, nullptr), "channel range", "sample: c1 < c0");

    refused(mpf_warp_composite_bwd(n, n, n, n, 4, 8, 8, n, n, n, nn, nn, nullptr), "null pointer", "fused: all null");
    refused(mpf_warp_composite_bwd(p, p, n, p, 4, 8, 8, p, n, n, p, nn, nullptr), "null pointer", "fused: no grad_sigma");
    refused(mpf_warp_composite_bwd(p, p, n, p, 4, 8, 8, n, n, n, p, p, nullptr), "null pointer", "fused: no g_rgb");
    refused(mpf_warp_composite_bwd(p, p, n, p, 0, 8, 8, p, n, n, p, p, nullptr), "bad shape", "fused: S = 0");
    refused(mpf_warp_composite_bwd(p, p, n, p, 4096, 8, 8, p, n, n, p, p, nullptr), "bad shape", "fused: S = 4096");
    refused(mpf_warp_composite_bwd(p, p, n, p, 4, 0, 8, p, n, n, p, p, nullptr), "bad shape", "fused: H = 0");
    refused(mpf_warp_composite_bwd(p, p, n, p, 4, 8, -1, p, n, n, p, p, nullptr), "bad shape", "fused: W < 0");
    refused(mpf_warp_composite_bwd(p, p, n, p, 4, 1 << 14, 1 << 14, p, n, n, p, p, nullptr), "too large", "fused: H*W = 2^28");
    refused(mpf_warp_composite_bwd(p, p, n, p, 4, 8, 8, p, n, p, p, p, nullptr), "quads", "fused: g_objmask without quads");
    refused(mpf_warp_composite_bwd(p, p, odd, p, 4, 8, 8, p, n, n, p, p, nullptr), "aligned", "fused: misaligned quads");

    if (g_failures) {
        fprintf(stderr, "%d of %d checks failed\n", g_failures, g_checks);
        return 1;
    }
    printf("ok: %d refusals\n", g_checks);
    return 0;
}

#include "fractalrenderer_amd.h"
#include <stdio.h>
#include <string.h>
/* fr_deep_sequence_plan under AddressSanitizer + UBSan, no device and no Python: every frame of the descriptors of
 * tests/test_deep_sequence_host.py, valid and rejected.  Links fr_deepseq.c, fr_deep.c and fr_host.c only:
 *   gcc -std=c11 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -Iinclude
 *       -Ifractalrenderer_amd/csrc tests/c_client/deepseq_plan_sweep.c fractalrenderer_amd/csrc/fr_deepseq.c
 *       fractalrenderer_amd/csrc/fr_deep.c fractalrenderer_amd/csrc/fr_host.c -lm -o deepseq_plan_sweep
 * Prints the number of descriptors accepted and rejected and of frames planned; exit status 0 when every frame of every
 * accepted descriptor has a mantissa in [1, 2) and u in (0.5, 1]. */
static const char* kCx = "-1.7499";      /* any centre: the plan reads it only to validate it */
static const char* kCy = "0.00000000000000000000000000000000000000000000000000000000000000000000000000000000000000000001";

int main(void)
{
    static const struct { const char* first; const char* last; int frames; } walks[] = {
        {"1e-110", "2.5e-111", 9}, {"2.5e-111", "1e-110", 9}, {"3e-20", "7e-25", 50}, {"1e-300", "2.5e-301", 5},
        {"3", "1e-400", 7}, {"1e-999", "2e-1000", 7}, {"1e-20", "1e-20", 7}, {"1.5e-1000", "1e-1000", 3},
        {"3e-1000", "1e-1000", 4}, {"600", "1000", 3}, {"4e-1000", "1e-1000", 9}, {"2e-1000", "1e-1000", 3},
        {"250", "1000", 5}, {"1e3", "1e-1000", 3001}, {"1e-1000", "1e3", 2}, {"1e-1001", "1", 4}, {"1", "1e4", 4},
        {"0", "1", 4}, {"x", "1", 4}, {"", "1", 4}, {NULL, "1", 4}, {"1", NULL, 4}, {"1e-110", "2.5e-111", 1},
        {"1e-110", "2.5e-111", 0}, {"1e-110", "2.5e-111", -3}, {"1e-110", "2.5e-111", 2},
    };
    static const int fracs[] = {0, 128, 640, 4096, -1, 1, 127, 4097};
    long accepted = 0, rejected = 0, frames = 0, bad = 0;
    for (size_t w = 0; w < sizeof walks / sizeof walks[0]; ++w)
        for (int mode = -1; mode <= 2; ++mode)
            for (size_t fb = 0; fb < sizeof fracs / sizeof fracs[0]; ++fb)
                for (int variant = 0; variant < 4; ++variant) {
                    fr_deep_sequence_desc d = {kCx, kCy, walks[w].first, walks[w].last, walks[w].frames, fracs[fb], mode, 0};
                    if (variant == 1) d.reserved = 1;
                    if (variant == 2) d.center_x = NULL;
                    if (variant == 3) d.center_y = "5e9";
                    fr_deep_sequence_frame f;
                    memset(&f, 0, sizeof f);
                    if (fr_deep_sequence_plan(&d, 0, &f) != FR_OK) { ++rejected; continue; }
                    ++accepted;
                    if (fr_deep_sequence_plan(&d, -1, &f) == FR_OK || fr_deep_sequence_plan(&d, d.frames, &f) == FR_OK) ++bad;
                    for (int i = 0; i < d.frames; ++i) {
                        if (fr_deep_sequence_plan(&d, i, &f) != FR_OK) { ++bad; continue; }
                        ++frames;
                        if (!(f.zoom_mant >= 1.0 && f.zoom_mant < 2.0) || !(f.u > 0.5 && f.u <= 1.0)) ++bad;
                        if (f.resampled != (mode == 1 && f.u != 1.0)) ++bad;
                    }
                }
    if (fr_deep_sequence_plan(NULL, 0, NULL) == FR_OK) ++bad;
    printf("descriptors accepted %ld rejected %ld, frames planned %ld, violations %ld\n", accepted, rejected, frames, bad);
    return bad ? 1 : 0;
}

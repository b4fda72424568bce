/* history_clamp_c99.c -- include/rustray_hip.h in a C99 translation unit: rr_history_clamp_params has the size and the offsets the header
 * states, its default call fills it without a device, and the two entry points refuse a NULL scene by name.
 * Built by tests/test_temporal_clamp_host.py with gcc -std=c99 -pedantic -Wall -Wextra -Werror. */
#include <stddef.h>
#include <stdio.h>
#include <string.h>

#include "../../include/rustray_hip.h"

typedef char size_is_12[sizeof(rr_history_clamp_params) == 12 ? 1 : -1];
typedef char struct_size_at_0[offsetof(rr_history_clamp_params, struct_size) == 0 ? 1 : -1];
typedef char radius_at_4[offsetof(rr_history_clamp_params, radius) == 4 ? 1 : -1];
typedef char sigma_scale_at_8[offsetof(rr_history_clamp_params, sigma_scale) == 8 ? 1 : -1];

int main(void) {
    rr_history_clamp_params c;
    rr_accumulate_params p;
    rr_camera cam;
    memset(&c, 0xff, sizeof c);
    memset(&cam, 0, sizeof cam);
    if (rr_history_clamp_default_params(NULL) != RR_ERR_INVALID_ARGUMENT) return 1;
    if (rr_history_clamp_default_params(&c) != RR_OK) return 2;
    if (c.struct_size != sizeof c || (c.radius != 1u && c.radius != 2u) || !(c.sigma_scale >= 0.0f && c.sigma_scale <= 65536.0f)) return 3;
    if (rr_accumulate_default_params(&p) != RR_OK) return 4;
    if (rr_accumulate_clamped_records(NULL, &cam, &p, &c, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != RR_ERR_INVALID_ARGUMENT) return 5;
    if (!strstr(rr_last_error(), "rr_accumulate_clamped_records: scene")) return 6;
    if (rr_accumulate_clamped_records_device(NULL, &cam, &p, &c, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != RR_ERR_INVALID_ARGUMENT) return 7;
    if (!strstr(rr_last_error(), "rr_accumulate_clamped_records_device: scene")) return 8;
    printf("history clamp c99 OK: radius %u, sigma_scale %g\n", (unsigned)c.radius, (double)c.sigma_scale);
    return 0;
}

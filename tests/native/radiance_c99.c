/* rr_radiance and rr_shade_rays of include/rustray_hip.h from a plain C99 host (compiled with -pedantic -Werror by
 * tests/test_shade_rays_host.py and linked against librustray_hip.so): the record's layout and the argument checks that
 * come before anything touches a scene.  Runs without a GPU. */
#include "../../include/rustray_hip.h"

#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, rr_last_error()); return 1; } } while (0)

int main(void) {
    rr_radiance out[2];
    rr_config cfg;
    float o[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, d[6] = {0.0f, 0.0f, -1.0f, 0.0f, 0.0f, -1.0f};

    CHECK(sizeof(rr_radiance) == 32);
    CHECK(offsetof(rr_radiance, color) == 0 && offsetof(rr_radiance, depth) == 12 && offsetof(rr_radiance, normal) == 16 && offsetof(rr_radiance, object_id) == 28);
    memset(&cfg, 0, sizeof cfg);
    memset(out, 0x5a, sizeof out);
    CHECK(rr_shade_rays(NULL, &cfg, o, d, 2u, 1u, NULL, out, NULL) == RR_ERR_INVALID_ARGUMENT);
    CHECK(strstr(rr_last_error(), "NULL") != NULL);
    CHECK(((unsigned char*)out)[0] == 0x5a && ((unsigned char*)out)[63] == 0x5a);
    printf("radiance c99 OK\n");
    return 0;
}

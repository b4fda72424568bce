/* rr_albedo_pixels / rr_albedo_pixels_device as a C99 host sees them (tests/test_abi_albedo_pixels.py): the header compiles as C99,
 * both symbols link, and every refusal that needs no device comes in the order the header states. */
#include "../../include/rustray_hip.h"

#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, rr_last_error()); return 1; } } while (0)

int main(void) {
    static float albedo[18];
    uint32_t list[2] = {0u, 1u | (1u << 16)};
    rr_camera cam;
    rr_config cfg;
    rr_scene* fake = (rr_scene*)(void*)albedo; /* never dereferenced: every call below is refused by its arguments alone */
    int k;

    memset(&cam, 0, sizeof cam);
    memset(&cfg, 0, sizeof cfg);
    cam.width = 3u; cam.height = 2u;
    cfg.samples = 4;
    for (k = 0; k < 4; k++) { cam.projection_inverse[5 * k] = 1.0f; cam.view_inverse[5 * k] = 1.0f; }
    memset(albedo, 0x5a, sizeof albedo);

    /* a NULL scene, camera or config comes first, whatever else is wrong */
    CHECK(rr_albedo_pixels(NULL, &cam, &cfg, NULL, NULL, 6u, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL argument") != NULL);
    CHECK(rr_albedo_pixels_device(NULL, &cam, &cfg, NULL, NULL, 6u, NULL, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL argument") != NULL);
    CHECK(rr_albedo_pixels(fake, NULL, &cfg, NULL, NULL, 6u, albedo, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL argument") != NULL);
    CHECK(rr_albedo_pixels(fake, &cam, NULL, NULL, NULL, 6u, albedo, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL argument") != NULL);
    /* the config is checked as a frame's */
    cfg.samples = 0;
    CHECK(rr_albedo_pixels(fake, &cam, &cfg, NULL, NULL, 6u, albedo, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "samples must be >= 1") != NULL);
    cfg.samples = 4;
    /* then the output */
    CHECK(rr_albedo_pixels(fake, &cam, &cfg, NULL, NULL, 5u, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "albedo_out is required") != NULL);
    CHECK(rr_albedo_pixels_device(fake, &cam, &cfg, NULL, NULL, 0u, NULL, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "albedo_out is required") != NULL);
    /* the pixel limit */
    CHECK(rr_albedo_pixels(fake, &cam, &cfg, NULL, list, (1u << 30) + 1u, albedo, NULL) == RR_ERR_UNSUPPORTED);
    CHECK(rr_albedo_pixels_device(fake, &cam, &cfg, NULL, list, (1u << 30) + 1u, albedo, NULL, NULL) == RR_ERR_UNSUPPORTED);
    /* n_pixels == 0: RR_OK, nothing is looked at */
    CHECK(rr_albedo_pixels(fake, &cam, &cfg, NULL, NULL, 0u, albedo, NULL) == RR_OK);
    CHECK(rr_albedo_pixels_device(fake, &cam, &cfg, NULL, list, 0u, albedo, NULL, NULL) == RR_OK);
    /* without a list n_pixels is the frame's */
    CHECK(rr_albedo_pixels(fake, &cam, &cfg, NULL, NULL, 5u, albedo, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "5 pixels without a list") != NULL);
    CHECK(rr_albedo_pixels_device(fake, &cam, &cfg, NULL, NULL, 7u, albedo, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "7 pixels without a list") != NULL);
    /* a list entry outside the frame is refused by the host form naming its index, before the scene is looked at */
    list[1] = 3u;
    CHECK(rr_albedo_pixels(fake, &cam, &cfg, NULL, list, 2u, albedo, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "pixel_xy[1] = (3, 0)") != NULL);
    { size_t b; for (b = 0; b < sizeof albedo; b++) CHECK(((unsigned char*)albedo)[b] == 0x5a); } /* and nothing was written */
    printf("albedo pixels c99 OK\n");
    return 0;
}

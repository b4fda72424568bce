/* rr_surface_pixels / rr_surface_pixels_device as a C99 host sees them (tests/test_abi_surface_pixels.py): the header compiles as C99,
 * both symbols link, and every refusal that needs no device comes in the order the header states. */
#include "../../include/rustray_hip.h"

#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, rr_last_error()); return 1; } } while (0)

int main(void) {
    static rr_surface_hit out[6];
    static float albedo[18];
    uint32_t list[2] = {0u, 1u | (1u << 16)};
    rr_camera cam;
    rr_scene* fake = (rr_scene*)(void*)out; /* never dereferenced: every call below is refused by its arguments alone */
    int k;

    memset(&cam, 0, sizeof cam);
    cam.width = 3u; cam.height = 2u;
    for (k = 0; k < 4; k++) { cam.projection_inverse[5 * k] = 1.0f; cam.view_inverse[5 * k] = 1.0f; }
    memset(out, 0x5a, sizeof out);
    memset(albedo, 0x5a, sizeof albedo);

    /* a NULL scene or camera comes first, whatever else is wrong */
    CHECK(rr_surface_pixels(NULL, &cam, NULL, 6u, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL argument") != NULL);
    CHECK(rr_surface_pixels_device(NULL, &cam, NULL, 6u, NULL, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL argument") != NULL);
    CHECK(rr_surface_pixels(fake, NULL, NULL, 6u, out, albedo) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL argument") != NULL);
    /* then both outputs NULL, before the frame's size is compared with n_pixels */
    CHECK(rr_surface_pixels(fake, &cam, NULL, 5u, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "both NULL") != NULL);
    CHECK(rr_surface_pixels_device(fake, &cam, NULL, 5u, NULL, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "both NULL") != NULL);
    CHECK(rr_surface_pixels(fake, &cam, NULL, 0u, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "both NULL") != NULL);
    /* the pixel limit */
    CHECK(rr_surface_pixels(fake, &cam, list, 0x7fffff01u, out, NULL) == RR_ERR_UNSUPPORTED);
    CHECK(rr_surface_pixels_device(fake, &cam, list, 0x7fffff01u, out, NULL, NULL) == RR_ERR_UNSUPPORTED);
    /* n_pixels == 0: RR_OK, nothing is looked at */
    CHECK(rr_surface_pixels(fake, &cam, NULL, 0u, out, NULL) == RR_OK);
    CHECK(rr_surface_pixels(fake, &cam, list, 0u, NULL, albedo) == RR_OK);
    CHECK(rr_surface_pixels_device(fake, &cam, NULL, 0u, out, albedo, NULL) == RR_OK);
    /* without a list n_pixels is the frame's */
    CHECK(rr_surface_pixels(fake, &cam, NULL, 5u, out, albedo) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "5 pixels without a list") != NULL);
    CHECK(rr_surface_pixels_device(fake, &cam, NULL, 7u, out, NULL, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "7 pixels without a list") != NULL);
    /* a list entry outside the frame is refused by the host form naming its index, before the scene is looked at */
    list[1] = 3u;
    CHECK(rr_surface_pixels(fake, &cam, list, 2u, out, albedo) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "pixel_xy[1] = (3, 0)") != NULL);
    { size_t b; for (b = 0; b < sizeof out; b++) CHECK(((unsigned char*)out)[b] == 0x5a); } /* and nothing was written */
    { size_t b; for (b = 0; b < sizeof albedo; b++) CHECK(((unsigned char*)albedo)[b] == 0x5a); }
    printf("surface pixels c99 OK\n");
    return 0;
}

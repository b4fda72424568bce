/* rr_surface_hit as a C99 host sees it (tests/test_surface_rays_host.py): the size and every field offset, one per line as
 * "name offset size", then the argument checks of rr_surface_rays / rr_surface_rays_device that need no device. */
#include "../../include/rustray_hip.h"

#include <stddef.h>
#include <stdio.h>
#include <string.h>

#define CHECK(c) do { if (!(c)) { printf("FAILED %s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, rr_last_error()); return 1; } } while (0)
#define FIELD(f) printf("%s %u %u\n", #f, (unsigned)offsetof(rr_surface_hit, f), (unsigned)sizeof(((rr_surface_hit*)0)->f))

int main(void) {
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, -1.0f};
    rr_surface_hit out;
    rr_scene* fake = (rr_scene*)(void*)&out; /* never dereferenced: every call below is refused by its arguments alone */

    printf("sizeof %u\n", (unsigned)sizeof(rr_surface_hit));
    FIELD(hit); FIELD(item_index); FIELD(object_id); FIELD(face_id);
    FIELD(position); FIELD(distance);
    FIELD(normal); FIELD(material);
    FIELD(shading_normal); FIELD(has_uv);
    FIELD(base_color);
    FIELD(ambient_color); FIELD(alpha);
    FIELD(specular_color); FIELD(reflectivity);
    FIELD(uv); FIELD(roughness); FIELD(ambient_occlusion);

    memset(&out, 0x5a, sizeof out);
    CHECK(rr_surface_rays(NULL, o, d, 1u, 1u, &out) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL") != NULL);
    CHECK(rr_surface_rays_device(NULL, o, d, 1u, 1u, &out, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL") != NULL);
    CHECK(rr_surface_rays(fake, o, d, 1u, 0u, &out) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "depth") != NULL);
    CHECK(rr_surface_rays(fake, o, d, 1u, 256u, &out) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "depth") != NULL);
    CHECK(rr_surface_rays_device(fake, o, d, 1u, 0u, &out, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "depth") != NULL);
    CHECK(rr_surface_rays_device(fake, o, d, 1u, 256u, &out, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "depth") != NULL);
    CHECK(rr_surface_rays(fake, NULL, d, 1u, 1u, &out) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL") != NULL);
    CHECK(rr_surface_rays(fake, o, NULL, 1u, 1u, &out) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL") != NULL);
    CHECK(rr_surface_rays(fake, o, d, 1u, 1u, NULL) == RR_ERR_INVALID_ARGUMENT && strstr(rr_last_error(), "NULL") != NULL);
    CHECK(rr_surface_rays_device(fake, NULL, d, 1u, 1u, &out, NULL) == RR_ERR_INVALID_ARGUMENT);
    CHECK(rr_surface_rays_device(fake, o, NULL, 1u, 1u, &out, NULL) == RR_ERR_INVALID_ARGUMENT);
    CHECK(rr_surface_rays_device(fake, o, d, 1u, 1u, NULL, NULL) == RR_ERR_INVALID_ARGUMENT);
    CHECK(rr_surface_rays(fake, o, d, 0x7fffff01u, 1u, &out) == RR_ERR_UNSUPPORTED);
    CHECK(rr_surface_rays_device(fake, o, d, 0x7fffff01u, 1u, &out, NULL) == RR_ERR_UNSUPPORTED);
    CHECK(rr_surface_rays(fake, NULL, NULL, 0u, 1u, NULL) == RR_OK);            /* n == 0: RR_OK, nothing is looked at */
    CHECK(rr_surface_rays_device(fake, NULL, NULL, 0u, 1u, NULL, NULL) == RR_OK);
    { size_t k; for (k = 0; k < sizeof out; k++) CHECK(((unsigned char*)&out)[k] == 0x5a); } /* and nothing was written */
    printf("surface c99 OK\n");
    return 0;
}

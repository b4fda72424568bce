// rr_api.hip — host side of librustray_hip.so: the C ABI of include/rustray_hip.h.
//
// Replaces the frame loop of `RendererManager::start` (reference
// src/renderer.rs:105-172): instead of a shuffled queue of 2x2-pixel cells and
// num_cpus-2 worker threads calling Raytracing::render per pixel, one call
// uploads the frame constants and drives the wavefront kernels of
// rr_kernels.hip over batches of primary samples.
//
// This file is the index of ONE translation unit: the system headers, the kernels, then the host layers in dependency order.
// Every layer file is included exactly once, here, and says at its top what it offers and what it needs from the files before it.
#include "../../include/rustray_hip.h"
#include "rr_bvh.h"
#include "rr_device.h"
#include "rr_frame_plan.h"
#include "rr_primary_setup.h"
#include "rr_query_pointers.h"
#include "rr_arg_ranges.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <initializer_list>
#include <new>
#include <stdexcept>
#include <limits>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>

#include "rr_kernels.hip"

#include "rr_api_base.h"     // errors, the no-throw guard, the test fault hook (and rr_scene_build.h behind it), DevBuf
#include "rr_sample_table.h" // the reference's sub-sample table; regions of a frame (no HIP call)
#include "rr_schedule_log.h" // the schedule recorder of a frame (off by default): the wrappers of its event and stream calls
#include "rr_api_handle.h"   // rr_scene in its parts, one per layer below
#include "rr_api_scene.h"    // scene creation, the view, the top level and its reach, in-place and structural edits
#include "rr_api_frame.h"    // the frame driver: level walk, level 1 in stages, stats, tuning
#include "rr_api_multi.h"    // one frame on several devices; the gather maps
#include "rr_api_post.h"     // post-processing
#include "rr_api_query.h"    // rr_pick; closest-hit, shadow, surface and radiance queries
#include "rr_api_parts.h"    // rr_render_pixel_parts: a pixel's samples as K interleaved means
#include "rr_api_adaptive.h" // rr_refine_list_device, rr_render_adaptive: find the noisy pixels and refine them on the device
#include "rr_api_levels.h"   // rr_refine_sublist_device, rr_render_adaptive_levels: the list of a list, and a frame refined level by level
#include "rr_api_prefix.h"   // rr_render_pixel_prefix, rr_render_adaptive_prefix: the first samples of a frame, and refined pixels that keep theirs
#include "rr_api_denoise.h"  // rr_denoise_records: the variance-guided a-trous filter over a frame of records
#include "rr_api_temporal.h" // rr_accumulate_records: temporal reprojection of a frame of records, the step before the filter
#include "rr_api_motion.h"   // rr_motion_records: the per-pixel motion of moved items, what the reprojection takes when the scene is animated
#include "rr_api_surface_pixels.h" // rr_surface_pixels: the G-buffer and the albedo of the camera's pixel-centre rays, what the filter takes as its albedo guide
#include "rr_api_albedo_pixels.h" // rr_albedo_pixels: the frame's albedo averaged over its sub-samples, the albedo guide that is right at an edge pixel
#include "rr_api_pixel_split.h" // rr_render_pixel_split: the frame's records and, as a sum of its own, the direct diffuse light of the primary hits
#include "rr_api_upsample.h" // rr_upsample_records: a frame traced at a low resolution raised to the full one by the G-buffer
#include "rr_api_probe.h"    // device arithmetic probe, developer counters
#include "rr_api_schedule_probe.h" // test entry points: switch the schedule recorder on, read its log back

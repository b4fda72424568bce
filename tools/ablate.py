#!/usr/bin/env python3
"""Developer tool: cost breakdown of a kernel by ABLATION (the pool refuses rocprofv3 PC sampling).  Builds the library from a patched
copy of csrc/ in which one piece of work is removed (the frame is then WRONG: only the kernel times of tools/ab.sh are read) into
build/lib_abl_<name>.so.  usage: tools/ablate.py <name> [<name> ...] | all"""
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rustray_amd.capi import LIB_SOURCES  # noqa: E402

K = "rr_kernels.hip"   # k_shade itself
S = "rr_surface.h"     # textures and jitter
PATCHES = {
    "nojit": [(S, "    if (spread <= 0.0f) return dir;\n    f3 b3 = normalize3(dir);", "    return dir;\n    f3 b3 = normalize3(dir);")],
    "nopow": [(K, "const float light_power = powf(spec_dot, m.shininess);", "const float light_power = spec_dot;")],
    "noaux": [(K, "        const bool with_aux = (acc.normal || acc.depth) && __ballot(aux_pix != 0xffffffffu) != 0ull;\n",
               "        if ((aux_nx ^ aux_ny ^ aux_nz ^ aux_d ^ (int)aux_pix) == 0x5a5a5a5b) acc.flags[0] = aux_pix;\n        const bool with_aux = false;\n")],
    # The merges and their atomics alone (round 24): every lane sum stays alive behind one runtime comparison, k_shade's and k_trace_shadow's.
    # (Round 3's "noacc" compared a 32-bit lane sum with a 64-bit constant: the test folded to false and took the shading with it.)
    "nomerge": [(K, "        const bool with_aux = (acc.normal || acc.depth) && __ballot(aux_pix != 0xffffffffu) != 0ull;\n",
                 "        if ((sum_r ^ sum_g ^ sum_b ^ aux_nx ^ aux_ny ^ aux_nz ^ aux_d ^ (int)sum_pix ^ (int)aux_pix) == 0x5a5a5a5b) acc.flags[0] = sum_pix;\n        const bool with_aux = false;\n"),
                (K, "        if constexpr (SPLIT || !PRIMARY) {\n            accum_merged_runs(acc, sum_pix, sum_r, sum_g, sum_b);\n            if constexpr (SPLIT) accum_merged_runs(dacc, dif_pix, dif_r, dif_g, dif_b);\n            if (with_aux) accum_aux_merged_runs(acc, aux_pix, aux_nx, aux_ny, aux_nz, aux_d);\n        } else if (with_aux) accum_hit_merged(acc, sum_pix, sum_r, sum_g, sum_b, aux_pix, aux_nx, aux_ny, aux_nz, aux_d); // (colour and aux sums in one merge)\n        else accum_merged(acc, sum_pix, sum_r, sum_g, sum_b);\n", "")],
    # k_shade with the colour sums and the aux sums merged by two calls, each with its own one-pixel test, instead of accum_hit_merged
    "twomerge": [(K, "        } else if (with_aux) accum_hit_merged(acc, sum_pix, sum_r, sum_g, sum_b, aux_pix, aux_nx, aux_ny, aux_nz, aux_d); // (colour and aux sums in one merge)\n        else accum_merged(acc, sum_pix, sum_r, sum_g, sum_b);\n",
                  "        } else { accum_merged(acc, sum_pix, sum_r, sum_g, sum_b); if (with_aux) accum_aux_merged(acc, aux_pix, aux_nx, aux_ny, aux_nz, aux_d); }\n")],
    "nomerge_sh": [(K, "        if constexpr (FIXED && !SPLIT) accum_merged(acc, sum_pix, sum_r, sum_g, sum_b);\n        else accum_merged_runs(acc, sum_pix, sum_r, sum_g, sum_b);\n        if constexpr (SPLIT) accum_merged_runs(dacc, sum_pix, dif_r, dif_g, dif_b);\n",
                    "        if ((sum_r ^ sum_g ^ sum_b ^ (int)sum_pix) == 0x5a5a5a5b) acc.flags[0] = sum_pix;\n")],
    "nosq": [(K, "                if (sq_fixed) sq_wrote |= 1u << lk;", "                if (false) sq_wrote |= 1u << lk;"),
             (K, "                sq.s0[si] = make_float4(so.x, so.y, so.z, limit);\n                sq.s1[si] = make_float4(sd.x, sd.y, sd.z, __uint_as_float((uint32_t)item_idx | (depth << 27)));\n                sq.s2[si] = make_float4(cr, cg, cb, __uint_as_float(pix));\n",
              "                if (so.x + sd.x + cr + cg + cb + limit == 12345.678f) sq.s0[si] = make_float4(so.y, so.z, sd.y, sd.z);\n")],
    "notex": [(S, "    if (!(m.flags & (RR_MF_TEX_SLOT0 << slot)) || !has_uv) return false; // slot bit = index >= 0 and width > 0", "    return false;")],
    "nochild": [(K, "        spawn_refl = reflectivity > 0.0f && may_recurse;", "        spawn_refl = false;"),
                (K, "        if (alpha < 1.0f && may_recurse) {\n            // create_transmission", "        if (alpha < -1.0f && may_recurse) {\n            // create_transmission")],
    "nolight": [(K, "            const DLight L = light_uniform(sc.lights, li); // (all three groups are requested before the type is tested)\n            if (L.type & 0x80u) continue; // disabled",
                 "            const DLight L = light_uniform(sc.lights, li);\n            if (L.type != 0x7fu) continue;")],
    # Round 26, the ceiling of hiding a packet's stores behind the next packet's first load.  Both arms trace NO level-1 shadow ray (every
    # validity word is written as zero, so k_trace_shadow<true> idles in both); "novalid" still writes the three 16-byte records per light
    # and the object id, "nostores" keeps them behind comparisons that never hold.  k_shade<true> of novalid minus that of nostores is what
    # those stores cost.  The dense queue of the deeper levels is untouched (its records are read back by k_trace_shadow<false>).
    "novalid": [(K, "                if (sq_fixed) sq_wrote |= 1u << lk;", "                if (false) sq_wrote |= 1u << lk;")],
    "nostores": [(K, "                if (sq_fixed) sq_wrote |= 1u << lk;", "                if (false) sq_wrote |= 1u << lk;"),
                 (K, "                sq.s0[si] = make_float4(so.x, so.y, so.z, limit);\n                sq.s1[si] = make_float4(sd.x, sd.y, sd.z, __uint_as_float((uint32_t)item_idx | (depth << 27)));\n                sq.s2[si] = make_float4(cr, cg, cb, __uint_as_float(pix));\n",
                  "                if (!sq_fixed || so.x + sd.x + cr + cg + cb + limit == 12345.678f) {\n                sq.s0[si] = make_float4(so.x, so.y, so.z, limit);\n                sq.s1[si] = make_float4(sd.x, sd.y, sd.z, __uint_as_float((uint32_t)item_idx | (depth << 27)));\n                sq.s2[si] = make_float4(cr, cg, cb, __uint_as_float(pix));\n                }\n"),
                 (K, "            if (object_id) object_id[pix] = it_id;", "            if (object_id && it_id == 0x5a5a5a5bu) object_id[pix] = it_id;")],
}


def build(name):
    d = tempfile.mkdtemp(prefix="abl_")
    try:
        os.makedirs(os.path.join(d, "rustray_amd", "csrc"))
        os.makedirs(os.path.join(d, "include"))
        for f in LIB_SOURCES:
            shutil.copy(os.path.join(ROOT, "rustray_amd", "csrc", f), os.path.join(d, "rustray_amd", "csrc", f))
        shutil.copy(os.path.join(ROOT, "include", "rustray_hip.h"), os.path.join(d, "include", "rustray_hip.h"))
        for part in name.split("+"):
            for f, old, new in PATCHES[part]:
                p = os.path.join(d, "rustray_amd", "csrc", f)
                s = open(p).read()
                if s.count(old) != 1:
                    raise SystemExit(f"{name}: pattern of {part} found {s.count(old)} times in {f}")
                open(p, "w").write(s.replace(old, new))
        out = os.path.join(ROOT, "build", f"lib_abl_{name}.so")
        subprocess.check_call(["hipcc", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-fno-slp-vectorize", "--offload-arch=gfx950", "-Wno-unused-function",
                               "-Wno-unused-variable", "-Wno-unused-but-set-variable", "-shared", "-o", out, "rr_api.hip", "rr_bvh.cpp"],
                              cwd=os.path.join(d, "rustray_amd", "csrc"))
        print("built", out)
    finally:
        shutil.rmtree(d, ignore_errors=True)


if __name__ == "__main__":
    names = sys.argv[1:]
    if names == ["all"]:
        names = list(PATCHES)
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    for n in names:
        build(n)

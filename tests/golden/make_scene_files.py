"""The reference's own scene files, byte for byte, for the loader tests (tests/test_host.py).

The loader tests run `rustray_amd.scene.load_scene` on the reference's JSON / OBJ / MTL / glTF files and the one texture
they name, and compare what it builds with the committed flat scenes in scenes/.  Those files are DATA (inputs of the
loader, nothing of the reference's source); this script stores them in `scene_files.npz`:
  * `paths`: the file names relative to the reference's root (scene/..., as the scene files themselves name them);
  * `f<i>`: the bytes of file i (uint8), compressed by np.savez_compressed.
`tests/test_host.py` writes them back into a temporary tree laid out like the reference's and loads from there.

Run where a checkout of the reference exists:
    RUSTRAY_REFERENCE=<reference root> python tests/golden/make_scene_files.py
"""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

FILES = (
    "scene/spheres.json",
    "scene/textures/earth/2k_earth_normal_map.jpg",   # the textured sphere of spheres.json
    "scene/monkey.json",
    "scene/models/monkey/monkey.obj",
    "scene/models/monkey/monkey.mtl",
    "scene/models/monkey/monkey.glb",
)


def write_tree(npz_path: str, root: str) -> str:
    """Unpacks `npz_path` under `root` (the layout of the reference's tree); returns `root`."""
    z = np.load(npz_path, allow_pickle=False)
    for i, rel in enumerate(z["paths"].tolist()):
        dst = os.path.join(root, rel)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        with open(dst, "wb") as f:
            f.write(z[f"f{i}"].tobytes())
    return root


if __name__ == "__main__":
    REF = os.environ.get("RUSTRAY_REFERENCE")
    if not REF:
        raise SystemExit("set RUSTRAY_REFERENCE to the root of a checkout of the reference")
    arrays = {"paths": np.array(FILES)}
    for i, rel in enumerate(FILES):
        with open(os.path.join(REF, rel), "rb") as f:
            arrays[f"f{i}"] = np.frombuffer(f.read(), dtype=np.uint8)
    out = os.path.join(HERE, "scene_files.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes,", len(FILES), "files")

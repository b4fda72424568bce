"""Writes the stand-in image of the `add_objects` fixture tree.

The tree is laid out like the reference's working directory, as far as Scene::add_ground_plane and Scene::add_environment_sphere
(reference src/scene.rs:1564-1578) read it:
  scene/floor_reflective.json   the reference's values (data: one plane and its material fields)
  scene/environment.json        the reference's values (data: one sphere, its material fields and the path of its ambient map)
  scene/textures/environment/footprint_court.jpg
                                NOT the reference's photograph: a small generated sky gradient with a sun blob, written by this
                                script, at the path environment.json names
Run from the repository root:  python tests/golden/add_objects/make_add_objects.py
"""
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def stand_in(w=64, h=32):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = y / (h - 1)
    sky = np.stack([0.35 + 0.4 * v, 0.55 + 0.3 * v, 0.95 - 0.25 * v], axis=-1)
    ground = np.stack([0.30 + 0.1 * np.sin(x / 5.0), 0.25 + 0.1 * np.cos(x / 7.0), 0.20 + 0.0 * x], axis=-1)
    img = np.where((v < 0.55)[..., None], sky, ground)
    sun = np.exp(-(((x - 0.7 * w) / 4.0) ** 2 + ((y - 0.2 * h) / 3.0) ** 2))
    img = np.clip(img + sun[..., None] * (1.0, 0.9, 0.6), 0.0, 1.0)
    return (img * 255.0 + 0.5).astype(np.uint8)


if __name__ == "__main__":
    path = os.path.join(HERE, "scene", "textures", "environment", "footprint_court.jpg")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(stand_in(), "RGB").save(path, quality=90)
    print(path, os.path.getsize(path), "bytes")

"""Writes tests/golden/walk_rays.json: the REFERENCE's own hit records (oracle/_ref/libpbr_ref.so —
Scene::Intersect / IntersectP of the unmodified sources) for the lattice rays of
tests/ref_scenes.py walk_fixture_rays(): rays with ±0 direction components, origins on box planes, waves
holding all eight sign octants, and tMax at the hit distance and one ulp either side.

  python tests/golden/make_walk_fixtures.py          (development container: needs the reference)

Layout (arrays base64, little endian; ref_scenes.load_walk_fixture reads it): "hit" and "any" are the
closest-hit and any-hit flags, one bit per ray (numpy packbits); "t" (<f4) and "prim" (<i2) hold
the hit distance and primitive of the rays whose closest-hit flag is set, in ray order."""
import base64
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import numpy as np  # noqa: E402

import ref_scenes as RS  # noqa: E402

OUT = os.path.join(HERE, "walk_rays.json")


def b64(a):
    return base64.b64encode(np.ascontiguousarray(a).tobytes()).decode()


def make():
    import ref_lib as R
    s, rays, classes = RS.walk_fixture_rays()
    hit = R.intersect(s, rays)
    anyhit = R.intersect(s, rays, any_hit=True)
    h = hit[:, 0] == 1
    assert hit[h, 2].max() < 2 ** 15
    out = {"scene_digest": RS.scene_digest(s), "rays_sha256": hashlib.sha256(rays.astype("<f4").tobytes()).hexdigest(),
           "n": int(len(rays)), "classes": classes,
           "hit": b64(np.packbits(h)), "t": b64(hit[h, 1].astype("<f4")), "prim": b64(hit[h, 2].astype("<i2")),
           "any": b64(np.packbits(anyhit[:, 0] == 1))}
    return json.dumps(out, indent=0, sort_keys=True) + "\n"


if __name__ == "__main__":
    txt = make()
    open(OUT, "w").write(txt)
    print(f"{OUT}: {len(txt)} bytes")

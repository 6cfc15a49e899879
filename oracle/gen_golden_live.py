"""Generate tests/golden/model_live_cs_wild_places.npz (BUILD CONTAINER ONLY).

TEST INFRASTRUCTURE (see oracle/__init__.py).  The batch of
`tests/test_oracle_model.py::test_oracle_matches_reference_live` -- two clouds (forest_cloud(77, 1500),
unit_ball_cloud(78, 900)) through the reference's own model files (cs-wild-places cfg, closed-form
'stress' weights, octree depth 7) -- with the reference's descriptors, so that the test also runs
where the reference tree is absent:

    tests/golden/model_live_cs_wild_places.npz
        n_points     (2,) points per cloud
        points       (sum n, 3) float32, the clouds exactly as the model's octree receives them
        descriptors  (2, 256) float32 -- reference `model(batch)['global']`

Usage:  python -m oracle.gen_golden_live
"""

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import                                   # noqa: E402
from oracle.testing import oracle_octree, synthetic_state_dict   # noqa: E402
from hotformerloc_amd import synthetic as syn                    # noqa: E402
from hotformerloc_amd.params import load_config                  # noqa: E402


def main():
    model, _ = ref_import.reference_model(
        os.path.join(ref_import.REFERENCE_ROOT, 'models', 'hotformerloc_cs-wild-places_cfg.txt'))
    syn.fill_synthetic_weights(model, 'stress')
    # the test rebuilds these weights from the package's own cfg where the reference is absent: they must be the same tensors
    params, _ = load_config('cs-wild-places')
    mine = synthetic_state_dict(params, 'stress')
    theirs = model.state_dict()
    assert list(mine) == list(theirs) and all(torch.equal(mine[k], theirs[k]) for k in mine)
    clouds = [syn.forest_cloud(77, 1500), syn.unit_ball_cloud(78, 900)]
    with torch.inference_mode():
        y = model({'octree': oracle_octree(clouds, 7)})['global'].numpy()
    path = os.path.join(ROOT, 'tests', 'golden', 'model_live_cs_wild_places.npz')
    np.savez_compressed(path, n_points=np.array([len(c) for c in clouds]),
                        points=np.concatenate(clouds, 0).astype(np.float32), descriptors=y.astype(np.float32))
    print(path, y.shape, '%.0f KB' % (os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()

"""The hand-made cases added to the scenes of tests/test_gpu_prep.py and tests/test_gpu_detected_table.py hold what they were
built for: asserted on the host's functions alone, without a device (the scenes' own assertions run here)."""
import numpy as np

import test_gpu_detected_table as T
import test_gpu_prep as P


def test_sky_scene_holds_its_hand_made_cases():
    images, cat, want = P.sky_scene()           # (asserts the even count with a gap, claimed + 5 == median, the nelec row)
    assert len(want) == len(cat) == 80 and want[13:16] == [False, False, False]


def test_the_pivoting_jacobian_needs_its_rows_exchanged():
    J = P.rotated_image(P.PIVOT_ANGLE).wcs_jacobian
    assert 0 < abs(J[0, 0]) < 1e-6 * abs(J[1, 0])
    J = P.rotated_image(0.3).wcs_jacobian
    assert abs(J[0, 0]) > abs(J[1, 0])          # (the older scene never exchanges them)


def test_tie_scene_distances_are_exact_and_equal():
    images, cats = T.tie_scene()
    want = T.host_path(images, cats, T.TIE_RADIUS, exact_distances=True)
    w = want["worlds"]
    for a, b, d in ((w[1][0], w[0][0], 5.0), (w[1][0], w[0][1], 5.0), (w[1][1], w[0][2], 6.0), (w[2][0], w[0][2], 3.0), (w[2][0], w[1][1], 3.0)):
        dx, dy = a - b
        assert np.hypot(dx, dy) == d == np.sqrt(dx * dx + dy * dy)
    assert want["detections"] == [[(0, 0), (1, 0)], [(0, 1)], [(0, 2), (2, 0)], [(1, 1)]]

"""CPU: ``SceneEdges``, the edge rows a ``VerifiedScene`` hands its multi-view stages, on a scene made by hand from CPU tensors at the smallest
shape that has every kind of row: two launches (2 pairs and 1 pair), a launch row without a model (``stats[:, 0] == 0``, NaN pose), and two
``extra`` edges, one with a model and one holding the verifier's failure tuple. Every column is compared with an array written out here."""

import numpy as np
import pytest
import torch

from gtsfm_amd.frontend.correspondence_generator.scene_edges import SceneEdges
from gtsfm_amd.frontend.correspondence_generator.verified_scene import VerifiedScene

NAN = float("nan")
FAILURE = (None, None, np.array([], dtype=np.uint64), 0.0)


def rotation_z(deg):
    c, s = np.cos(np.radians(deg)), np.sin(np.radians(deg))
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


R01, R02, R23 = rotation_z(10.0), rotation_z(25.0), rotation_z(-40.0)
T01, T02, T23 = np.array([1.0, 0.0, 0.0]), np.array([0.0, 0.6, 0.8]), np.array([0.0, 0.0, -1.0])
CORR23 = np.array([[0, 1], [2, 3], [4, 5], [6, 7]], dtype=np.int64)


def launch(pairs, rotations, directions, counts):
    stats = np.zeros((len(pairs), 8), np.int32)
    stats[:, 0] = counts
    return {"pairs": pairs, "R": torch.from_numpy(np.stack(rotations)), "t": torch.from_numpy(np.stack(directions)), "stats": torch.from_numpy(stats)}


def make_scene(with_launches=True, with_extra=True):
    launches, verified, extra = [], {}, {}
    if with_launches:
        launches = [launch([(0, 1), (1, 2)], [R01, np.full((3, 3), NAN)], [T01, np.full(3, NAN)], [12, 0]), launch([(0, 2)], [R02], [T02], [7])]
        verified.update({(0, 1): (R01, T01, np.zeros((12, 2), np.int64), 0.8), (1, 2): FAILURE, (0, 2): (R02, T02, np.zeros((7, 2), np.int64), 0.6)})
    if with_extra:  # the edge without a model comes first: it leaves no row and does not shift the other
        verified.update({(1, 3): FAILURE, (2, 3): (R23, T23, CORR23, 0.5)})
        extra = {(1, 3): FAILURE[2], (2, 3): CORR23}
    return VerifiedScene([], {p: None for p in verified}, verified, {"xy": torch.zeros((4, 8, 2), dtype=torch.float32)}, launches, extra)


def assert_column(tensor, expected, dtype):
    assert tensor.dtype == dtype and tensor.is_contiguous() and tensor.device.type == "cpu"
    got = tensor.numpy()
    assert got.shape == expected.shape
    np.testing.assert_array_equal(got, expected)  # NaN equals NaN here


def test_every_column_equals_the_rows_written_out():
    table = make_scene().edge_table
    assert table.pairs == [(0, 1), (1, 2), (0, 2), (2, 3)] and table.num_images == 4
    assert_column(table.pair_images, np.array([[0, 1], [1, 2], [0, 2], [2, 3]], np.int32), torch.int32)
    assert_column(table.rotation, np.stack([R01.reshape(9), np.full(9, NAN), R02.reshape(9), R23.reshape(9)]), torch.float64)
    assert_column(table.direction, np.stack([T01, np.full(3, NAN), T02, T23]), torch.float64)
    assert_column(table.count, np.array([12.0, 0.0, 7.0, 4.0]), torch.float64)
    assert_column(table.has_model, np.array([1, 0, 1, 1], np.uint8), torch.uint8)


def test_mask_restricts_has_model_to_the_edges_given():
    table = make_scene().edge_table
    assert_column(table.mask(None), np.array([1, 0, 1, 1], np.uint8), torch.uint8)
    assert_column(table.mask([(0, 2), (2, 3)]), np.array([0, 0, 1, 1], np.uint8), torch.uint8)
    assert_column(table.mask({(0, 1), (1, 2), (5, 6)}), np.array([1, 0, 0, 0], np.uint8), torch.uint8)  # (1, 2) has no model, (5, 6) is no edge
    assert_column(table.mask(np.array([[2, 3]])), np.array([0, 0, 0, 1], np.uint8), torch.uint8)
    assert_column(table.has_model, np.array([1, 0, 1, 1], np.uint8), torch.uint8)  # the masks are new tensors


def test_a_scene_of_extra_edges_only():
    table = make_scene(with_launches=False).edge_table
    assert table.pairs == [(2, 3)]
    assert_column(table.pair_images, np.array([[2, 3]], np.int32), torch.int32)
    assert_column(table.rotation, R23.reshape(1, 9), torch.float64)
    assert_column(table.direction, T23.reshape(1, 3), torch.float64)
    assert_column(table.count, np.array([4.0]), torch.float64)
    assert_column(table.has_model, np.array([1], np.uint8), torch.uint8)
    assert_column(table.mask([(1, 3)]), np.array([0], np.uint8), torch.uint8)


def test_a_scene_without_rows():
    table = make_scene(with_launches=False, with_extra=False).edge_table
    assert table.pairs == []
    assert_column(table.pair_images, np.zeros((0, 2), np.int32), torch.int32)
    assert_column(table.rotation, np.zeros((0, 9)), torch.float64)
    assert_column(table.direction, np.zeros((0, 3)), torch.float64)
    assert_column(table.count, np.zeros(0), torch.float64)
    assert_column(table.has_model, np.zeros(0, np.uint8), torch.uint8)
    assert_column(table.mask(None), np.zeros(0, np.uint8), torch.uint8)
    assert_column(table.mask([(0, 1)]), np.zeros(0, np.uint8), torch.uint8)


def test_the_table_is_built_once_per_scene_and_a_column_once_when_asked_for(monkeypatch):
    built, columns = [], []
    init, column = SceneEdges.__init__, SceneEdges._column
    monkeypatch.setattr(SceneEdges, "__init__", lambda self, *a: (built.append(1), init(self, *a))[1])
    monkeypatch.setattr(SceneEdges, "_column", lambda self, *a: (columns.append(a[2:]), column(self, *a))[1])
    scene = make_scene()
    assert built == []
    table = scene.edge_table
    assert scene.edge_table is table and built == [1]
    assert columns == [] and not {"pair_images", "rotation", "direction", "count", "has_model"} & set(vars(table))  # nothing is built before it is asked for
    rotation = table.rotation
    assert table.rotation is rotation and columns == [(torch.float64, (9,))]
    assert table.mask(None) is table.has_model and table.mask([(0, 1)]) is not table.has_model and columns == [(torch.float64, (9,)), (torch.uint8,)]
    assert "direction" not in vars(table) and "count" not in vars(table)  # what the view graph does not read is not uploaded
    assert table.pair_images is table.pair_images


def test_another_scene_over_the_same_launches_has_its_own_table():
    scene = make_scene()
    table = scene.edge_table
    verified = dict(scene.verified)
    verified[(2, 3)] = FAILURE  # as two_view's result: the same launches, another host record
    verified[(1, 3)] = (R23, T23, CORR23[:2], 0.5)
    other = VerifiedScene(scene.keypoints_list, scene.putative, verified, scene.feats, list(scene.launches), {(1, 3): CORR23[:2], (2, 3): FAILURE[2]})
    assert other.edge_table is not table and scene.edge_table is table
    assert other.edge_table.pairs == [(0, 1), (1, 2), (0, 2), (1, 3)] and table.pairs == [(0, 1), (1, 2), (0, 2), (2, 3)]
    assert_column(other.edge_table.count, np.array([12.0, 0.0, 7.0, 2.0]), torch.float64)
    assert_column(table.count, np.array([12.0, 0.0, 7.0, 4.0]), torch.float64)


@pytest.mark.parametrize("rotation, direction", [(None, T23), (R23, None)])
def test_an_extra_edge_needs_both_a_rotation_and_a_direction(rotation, direction):
    scene = make_scene()
    scene.verified[(2, 3)] = (rotation, direction, CORR23, 0.5)  # no producer in the package leaves such a tuple; the table's rule is still one rule
    assert scene.edge_table.pairs == [(0, 1), (1, 2), (0, 2)]

"""CPU: the host side of de-duplicated image batches (config key `image_dedup`, batch key `image_index`): the collate per distinct
image against the plain collate, the index tables of ops.image_groups, and the numpy model the GPU tests hold the two kernels to
(tests/dedup_model.py) against a float64 sum."""
import numpy as np
import pytest
import torch

import dedup_model as M
from arrow_util import HashTokenizer, write_split
from m3ae_amd import config, data, ops


def _dataset(tmp_path, image_transform="host"):
    root = str(tmp_path / "arrows")
    write_split(root, "train", 7)   # images 2 and 5 carry three questions each, 1 and 4 two
    stats = data.TransformStats()
    ds = data.ArrowVQADataset(root, "train", 64, 32, HashTokenizer(), image_transform=image_transform, stats=stats)
    return ds, stats


def _same(a, b, key):
    if isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), key
    else:
        assert a == b, key


def test_collate_per_distinct_image_equals_the_plain_collate(tmp_path):
    ds, stats = _dataset(tmp_path)
    by_row = {}
    for i, (row, _) in enumerate(ds.index_mapper):
        by_row.setdefault(row, []).append(i)
    assert max(len(v) for v in by_row.values()) >= 3
    # all questions of rows 2, 5 and 1, one of row 0 and one of row 3, interleaved and out of order
    idx = [by_row[2][0], by_row[5][2], by_row[0][0], by_row[2][2], by_row[1][1], by_row[5][0], by_row[2][1], by_row[3][0],
           by_row[1][0], by_row[5][1]]
    plain = data.collate_host([ds[i] for i in idx], pin=False)
    n_plain = stats.decodes
    assert n_plain == len(idx)
    dedup = data.collate_dedup(ds, idx, pin=False)
    n_dedup = stats.decodes - n_plain
    rows = [ds.index_mapper[i][0] for i in idx]
    U = len(set(rows))
    assert U == 5 and n_dedup == U                       # one decode per distinct image row
    assert dedup["image_u8"].shape[0] == U
    ii = dedup["image_index"]
    assert ii.dtype == torch.int64 and ii.shape == (len(idx),)
    assert torch.equal(dedup["image_u8"][ii], plain["image_u8"])   # byte for byte
    first = {}
    assert ii.tolist() == [first.setdefault(r, len(first)) for r in rows]   # image rows in order of first use
    assert set(dedup) == set(plain) | {"image_index", "image_groups"}
    for k in plain:
        if k != "image_u8":
            _same(plain[k], dedup[k], k)
    g = dedup["image_groups"]
    off, mem = M.groups_of(ii.numpy(), U)
    assert g.n_images == U and not g.identity
    assert g.offsets.tolist() == off.tolist() and g.members.tolist() == mem.tolist() and torch.equal(g.index, ii)
    # the dataset's own contract is untouched: the sibling accessor returns the same sample minus the image, plus its key
    s, (sample, key) = ds[idx[0]], ds.sample_without_image(idx[0])
    assert set(s) == set(sample) | {"image_u8"} and all(s[k] == sample[k] for k in sample) and key[1] == 2
    assert np.array_equal(ds.image_by_key(key), s["image_u8"])


def test_collate_per_distinct_image_packs_the_sources_of_the_device_transform_once(tmp_path):
    ds, stats = _dataset(tmp_path, "device")
    idx = [i for i, (row, _) in enumerate(ds.index_mapper) if row in (2, 4, 5)]
    plain = data.collate_host([ds[i] for i in idx], pin=False, resample_size=64)
    dedup = data.collate_dedup(ds, idx, pin=False, resample_size=64)
    assert plain["image_u8"]["plan"].shape[0] == len(idx) == 8 and dedup["image_u8"]["plan"].shape[0] == 3
    assert stats.decodes == 8 + 3 and dedup["image_index"].tolist() == [0, 0, 0, 1, 1, 2, 2, 2]


def test_flag_defaults_off_and_is_refused_with_per_sample_image_objectives(tmp_path):
    assert config.DEFAULTS["image_dedup"] is False
    root = str(tmp_path / "arrows")
    write_split(root, "train", 3)
    cfg = config.tiny_config(data_root=root, per_gpu_batchsize=2, image_dedup=True)
    cfg["loss_names"] = dict(cfg["loss_names"], itm=1)
    with pytest.raises(ValueError, match="image_dedup"):
        data.ArrowDataModule(cfg, 0, 1, "cpu", tokenizer=HashTokenizer())


@pytest.mark.parametrize("index,identity", [([2, 0, 2, 1, 2], False), ([0, 0, 0, 0], False), (list(range(6)), True)])
def test_group_tables(index, identity):
    g = ops.image_groups(torch.tensor(index))
    off, mem = M.groups_of(index)
    assert g.n_images == len(off) - 1 == max(index) + 1 and g.n_samples == len(index) and g.identity is identity
    assert all(t.dtype == torch.int64 and t.is_contiguous() for t in g.tensors())
    assert g.index.tolist() == index and g.offsets.tolist() == off.tolist() and g.members.tolist() == mem.tolist()
    for u in range(g.n_images):   # every image's samples, ascending
        ms = g.members[g.offsets[u]:g.offsets[u + 1]].tolist()
        assert ms == sorted(ms) == [b for b, v in enumerate(index) if v == u]


def test_group_tables_refuse_an_unused_image_row_and_indices_out_of_range():
    with pytest.raises(ValueError, match="used by no sample"):
        ops.image_groups(torch.tensor([0, 2, 2, 0]))          # row 1 unused
    with pytest.raises(ValueError, match="used by no sample"):
        ops.image_groups(torch.tensor([0, 1]), n_images=3)
    with pytest.raises(ValueError, match="outside"):
        ops.image_groups(torch.tensor([0, 1, 3]), n_images=3)
    with pytest.raises(ValueError, match="outside"):
        ops.image_groups(torch.tensor([0, -1]))
    # a permutation is no identity
    assert not ops.image_groups(torch.tensor([1, 0, 2])).identity


@pytest.mark.parametrize("positive", [False, True])
def test_numpy_model_of_the_segment_sum_is_within_one_bf16_ulp_of_the_rounded_float64_sum(positive):
    """A check on the model itself: float32 adds in member order and one round-to-nearest-even against the float64 sum rounded
    to bf16 -- at most one bf16 ulp apart."""
    rng = np.random.RandomState(5)
    index = [0, 1, 2, 1, 2, 2, 2, 2, 2, 2]               # groups of 1, 2 and 7
    off, mem = M.groups_of(index)
    x = rng.standard_normal((len(index), 4096)).astype(np.float32)
    d = M.bf16_round(np.abs(x) + 0.5 if positive else x)
    got = M.bf16_to_f32(M.segment_sum(d, off, mem, bf16=True)).astype(np.float64)
    s64 = M.segment_sum_f64(d, off, mem, bf16=True)
    want = M.bf16_to_f32(M.bf16_round(s64.astype(np.float32))).astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(want), 2.0 ** -126))) - 7)
    assert (np.abs(got - want) <= ulp).all(), float((np.abs(got - want) / ulp).max())
    # the group of one is a copy, and the rounding is to nearest even
    assert np.array_equal(M.segment_sum(d, off, mem, bf16=True)[0], d[0])
    assert M.bf16_round(np.array([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20], dtype=np.float32)).tolist() \
        == [0x3F80, 0x3F82, 0x3F81]

"""The device-resident dataset cache on the MI355X (device_cache, csrc/cache.hip) against torch
on the CPU.  Every comparison is bit equality: the cache stores exactly or says so."""
import copy

import pandas as pd
import pytest
import torch
import torch.nn.functional as F

import multimodal_alzheimer_amd as M
from multimodal_alzheimer_amd import device_cache as dc, nifti
from multimodal_alzheimer_amd.data_parallel import ShardSampler
from multimodal_alzheimer_amd.preprocess import NORM_SPEC_KEY

pytestmark = pytest.mark.gpu

# odd W, a voxel count that is no multiple of 32, strides that need rounding; then the aligned case
SHAPES = [(5, 7, 67), (9, 11, 13), (16, 16, 16)]
N, B = 5, 3
INDICES = [4, 0, 4]                 # a repeat, the first slot and the last
_DATA = {}


def _data(shape):
    """float64 volumes that need all 53 bits, the same rounded to float32, a binary mask"""
    if shape not in _DATA:
        g = torch.Generator().manual_seed(sum(shape))
        x64 = torch.randn((N,) + shape, dtype=torch.float64, generator=g) * 100.0
        x64[0, 0, 0, :3] = torch.tensor([0.0, -0.0, 1e-30], dtype=torch.float64)
        x32 = x64.float().double()
        mask = (torch.rand((N,) + shape, generator=g) > 0.4).double()
        _DATA[shape] = (x64, x32, mask, torch.arange(N) % 3)
    return _DATA[shape]


def _same_bits(a, b):
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float64 and \
        torch.equal(a.view(torch.int64), b.view(torch.int64))


def _centre(x, out_shape):
    """the centre rule through F.pad: offset = floor((out - in) / 2) in front, the rest behind;
    negative pads crop"""
    pads = []
    for o, i in zip(reversed(out_shape), reversed(x.shape[-3:])):
        front = (o - i) // 2
        pads += [front, (o - i) - front]
    return F.pad(x, pads)


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("storage", ["float64", "float32", "float16"])
def test_store_and_fetch_round_trip(shape, storage):
    x64, x32, _, label = _data(shape)
    if storage == "float64":
        src, want = x64, x64
        cache = dc.DeviceVolumeCache.from_tensors(label, mri=src, storage=storage)
    elif storage == "float32":
        src, want = x32, x32
        cache = dc.DeviceVolumeCache.from_tensors(label, mri=src, storage=storage)
    else:
        src, want = x64, x64.half().double()
        with pytest.raises(dc.CacheInexact):
            dc.DeviceVolumeCache.from_tensors(label, mri=src, storage=storage)
        cache = dc.DeviceVolumeCache.from_tensors(label, mri=src, storage=storage, lossy=True)
        assert cache.mismatches["mri"] == int((want.view(torch.int64)
                                               != src.view(torch.int64)).sum())
    assert cache.storage == storage and cache.passes == 1
    vox = shape[0] * shape[1] * shape[2]
    assert cache.store_bytes("mri") == N * dc.scan_stride_bytes(vox, storage)
    got = cache.fetch(INDICES)
    assert list(got) == ["mri", "label"]
    assert _same_bits(got["mri"], want[INDICES])
    assert torch.equal(got["label"].cpu(), label[INDICES]) and got["label"].dtype == torch.int64
    every = cache.fetch(torch.arange(N))
    assert _same_bits(every["mri"], want)
    assert not cache.bad_index_seen()
    with pytest.raises(IndexError):
        cache.fetch([0, N])


@pytest.mark.parametrize("shape", SHAPES)
def test_auto_picks_the_narrowest_exact_dtype(shape):
    _, x32, _, label = _data(shape)
    cache = dc.DeviceVolumeCache.from_tensors(label, mri=x32, pet1451=x32.flip(0))
    assert cache.storage == "float32" and cache.passes == 1
    assert cache.mismatches == {"pet1451": 0, "mri": 0}
    got = cache.fetch(INDICES)
    assert _same_bits(got["mri"], x32[INDICES])
    assert _same_bits(got["pet1451"], x32.flip(0)[INDICES])

    x = x32.clone()
    x[3, -1, -1, -1] = 1.0 + 2.0 ** -40
    cache = dc.DeviceVolumeCache.from_tensors(label, mri=x)
    assert cache.storage == "float64" and cache.passes == 2
    assert _same_bits(cache.fetch(INDICES)["mri"], x[INDICES])
    with pytest.raises(dc.CacheInexact) as e:
        dc.DeviceVolumeCache.from_tensors(label, mri=x, storage="float32")
    assert e.value.mismatches == 1 and e.value.per_key == {"mri": 1}


@pytest.mark.parametrize("shape", SHAPES)
def test_masks_are_bits_when_binary(shape):
    _, x32, mask, label = _data(shape)
    vox = shape[0] * shape[1] * shape[2]
    cache = dc.DeviceVolumeCache.from_tensors(label, mri=x32, mri_mask=mask)
    assert cache.mask_storage == "bits" and cache.passes == 1
    assert cache.store_bytes("mri_mask") == N * dc.mask_stride_bytes(vox) \
        == N * ((-(-vox // 8) + 15) // 16 * 16)
    got = cache.fetch(INDICES)
    assert list(got) == ["mri", "mri_mask", "label"]
    assert _same_bits(got["mri_mask"], mask[INDICES]) and _same_bits(got["mri"], x32[INDICES])

    soft = mask.clone()
    soft[2, 1, 2, 3] = 0.5
    cache = dc.DeviceVolumeCache.from_tensors(label, mri=x32, mri_mask=soft)
    assert cache.mask_storage == cache.storage == "float32" and cache.passes == 2
    assert cache.store_bytes("mri_mask") == N * dc.scan_stride_bytes(vox, "float32")
    assert _same_bits(cache.fetch(INDICES)["mri_mask"], soft[INDICES])


@pytest.mark.parametrize("shape,out_shape", [((5, 7, 67), (8, 16, 64)),     # pad D, H; crop W
                                             ((9, 11, 13), (9, 11, 13)),    # identity
                                             ((16, 16, 16), (12, 20, 16)),
                                             # odd W': output rows alternate between 16-byte
                                             # aligned and 8 bytes off (row heads and tails)
                                             ((9, 11, 13), (11, 9, 15)),
                                             ((5, 7, 67), (5, 7, 33))])
@pytest.mark.parametrize("storage", ["float64", "float32", "float16"])
def test_pad_and_crop_by_the_centre_rule(shape, out_shape, storage):
    x64, x32, mask, label = _data(shape)
    src = {"float64": x64, "float32": x32, "float16": x64}[storage]
    want = x64.half().double() if storage == "float16" else src
    cache = dc.DeviceVolumeCache.from_tensors(label, mri=src, mri_mask=mask, storage=storage,
                                              out_shape=out_shape, lossy=storage == "float16")
    got = cache.fetch(INDICES)
    assert got["mri"].shape == (B,) + out_shape
    assert _same_bits(got["mri"], _centre(want[INDICES], out_shape))
    assert _same_bits(got["mri_mask"], _centre(mask[INDICES], out_shape))
    # a mask kept as values takes the same path as the volume
    soft = mask.clone()
    soft[0, 0, 0, 0] = 0.5
    cache = dc.DeviceVolumeCache.from_tensors(label, mri=x32, mri_mask=soft, out_shape=out_shape)
    assert _same_bits(cache.fetch(INDICES)["mri_mask"], _centre(soft[INDICES], out_shape))
    assert not cache.bad_index_seen()


def _nifti_table(tmp_path, n=7, shape=(9, 11, 13)):
    """PET + MRI + brain mask per subject, three classes (as tests/test_preprocess_gpu.py
    builds its scans: integer-valued MRI, uint8 mask)"""
    g = torch.Generator().manual_seed(5)
    rows = []
    for b in range(n):
        mri = torch.randint(0, 4096, shape, generator=g).double()
        pet = torch.rand(shape, generator=g)                       # float32 on disk
        mask = (torch.rand(shape, generator=g) > 0.3).to(torch.uint8)
        paths = [str(tmp_path / f"{k}{b}.nii{'.gz' if k == 'mri' else ''}")
                 for k in ("mri", "pet", "mask")]
        nifti.save(paths[0], mri.numpy())
        nifti.save(paths[1], pet.numpy())
        nifti.save(paths[2], mask.numpy())
        rows.append({"ID": f"sub-{b}", "ses": "2019-05-01", "path_anat": paths[0],
                     "path_pet1451": paths[1], "path_anat_mask": paths[2],
                     "label": ("CN", "MCI", "Dementia")[b % 3]})
    csv = tmp_path / "table.csv"
    pd.DataFrame(rows).to_csv(csv)
    return str(csv)


def _to_dev(batch):
    return {k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()}


def _assert_same_batch(got, want):
    assert list(got) == list(want)
    for k in want:
        if torch.is_tensor(want[k]):
            assert got[k].dtype == want[k].dtype and got[k].device == want[k].device, k
            assert torch.equal(got[k], want[k]), k
        else:
            assert list(got[k]) == list(want[k]), k


def test_feed_equals_the_sharded_dataloader(tmp_path):
    from multimodal_alzheimer_amd.dataset import MultiModalDataset
    ds = MultiModalDataset(_nifti_table(tmp_path), modalities=["pet1451", "t1w"],
                           normalize_mri={"per_scan_norm": "min_max"}, quantile=0.98,
                           device_normalize=True)
    assert len(ds) == 7
    cache = dc.DeviceVolumeCache.from_dataset(ds, "cuda")
    assert cache.storage == "float32" and cache.mask_storage == "bits" and cache.passes == 1
    assert cache.keys == ("pet1451", "mri", "mri_mask", "label")
    bs, seed = 2, 31
    for world in (1, 2):
        for rank in range(world):
            sampler = ShardSampler(ds, rank=rank, world=world, shuffle=True, seed=seed)
            loader = torch.utils.data.DataLoader(ds, batch_size=bs, sampler=sampler,
                                                 drop_last=True)
            feed = cache.feed(bs, rank=rank, world=world, shuffle=True, seed=seed)
            for epoch in (0, 1):
                sampler.set_epoch(epoch)
                want = [_to_dev(b) for b in loader]
                assert feed.epoch == epoch or feed.step == len(feed)
                got = list(feed)
                assert feed.epoch == epoch and len(got) == len(want) == len(feed)
                for g, w in zip(got, want):
                    _assert_same_batch(g, w)
                    assert NORM_SPEC_KEY in g
                    gp, wp = M.Base_Model.prepare_batch(g), M.Base_Model.prepare_batch(w)
                    assert set(gp) == set(wp) == {"pet1451", "mri", "label"}
                    assert torch.equal(gp["mri"], wp["mri"])
                    assert torch.equal(gp["pet1451"], wp["pet1451"])
    # without drop_last the last batch is short, as the loader's
    feed = cache.feed(bs, shuffle=False, drop_last=False)
    loader = torch.utils.data.DataLoader(ds, batch_size=bs, shuffle=False)
    got, want = list(feed), [_to_dev(b) for b in loader]
    assert [g["label"].shape[0] for g in got] == [2, 2, 2, 1]
    for g, w in zip(got, want):
        _assert_same_batch(g, w)
    assert not cache.bad_index_seen()


def test_captured_fetch_moves_on_with_the_cursor():
    shape = (9, 11, 13)
    _, x32, mask, label = _data(shape)
    tab = torch.arange(N * 9, dtype=torch.float32).reshape(N, 9) / 7
    n7 = torch.arange(7) % N                         # 7 samples: 3 batches of 2 per epoch
    cache = dc.DeviceVolumeCache.from_tensors(label[n7], mri=x32[n7], pet1451=x32[n7].flip(1),
                                              mri_mask=mask[n7], tabular=tab[n7],
                                              out_shape=(10, 10, 12))
    feed = cache.feed(2, shuffle=True, seed=3).prepare()
    static = cache.empty_batch(2)
    assert static["tabular"].dtype == torch.float32
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        feed.fetch_into(static)

    def replay_and_check(epoch, step):
        feed.before_replay()
        g.replay()
        assert (feed.epoch, feed.step) == (epoch, step + 1)
        want = cache.fetch(feed.epoch_batches(epoch)[step])
        _assert_same_batch({k: v for k, v in static.items()}, want)
        idx = feed.epoch_batches(epoch)[step]
        assert _same_bits(static["mri"], _centre(x32[n7][idx], (10, 10, 12)))
        assert torch.equal(static["tabular"].cpu(), tab[n7][idx])

    assert len(feed) == 3
    for step in range(3):
        replay_and_check(0, step)
    feed.next_epoch()
    for step in range(3):
        replay_and_check(1, step)
    replay_and_check(2, 0)                           # the feed rolls the epoch over by itself
    assert feed.epoch_batches(0) != feed.epoch_batches(1)
    assert not cache.bad_index_seen()


def _hparams():
    return {"n_classes": 2, "resnet_depth": 10, "conv_out": [], "filter_size": [],
            "batchnorm_begin": False, "batchnorm_dense": False, "linear_out": [],
            "fl_gamma": None, "lr": 1e-3, "lr_pretrained": 1e-5, "l2_reg": 0,
            "reduce_factor_lr_schedule": None, "precision": "bf16",
            "loss_class_weights": torch.tensor([0.3, 0.7], dtype=torch.float64)}


def test_graphed_step_fed_by_the_cache_equals_explicit_batches():
    """GraphedTrainStep(feed=...) replayed four times (one epoch, fetched inside the graph) and a
    GraphedTrainStep handed the same four batches: identical losses and parameters."""
    from multimodal_alzheimer_amd.graph_step import GraphedTrainStep
    g = torch.Generator().manual_seed(9)
    n, s, bs, warm = 9, 32, 2, 2
    x = torch.rand((n, s, s, s), dtype=torch.float64, generator=g)
    y = torch.randint(0, 2, (n,), generator=g)
    cache = dc.DeviceVolumeCache.from_tensors(y, mri=x)
    assert cache.storage == "float64"
    feed = cache.feed(bs, shuffle=True, seed=4)
    assert len(feed) == 4
    batches = [cache.fetch(i) for i in feed.epoch_batches(0)]
    torch.manual_seed(3)
    a = M.Anat_CNN(_hparams()).cuda()
    b = copy.deepcopy(a)

    gs_a = GraphedTrainStep(a, a.configure_optimizers(), batches[0], warmup=warm)
    losses_a = [gs_a(batches[i])["loss"].clone() for i in range(4)]
    gs_b = GraphedTrainStep(b, b.configure_optimizers(), warmup=warm, feed=feed)
    losses_b = []
    for i in range(4):
        losses_b.append(gs_b()["loss"].clone())
        assert torch.equal(gs_b.static["mri"], batches[i]["mri"])
        assert torch.equal(gs_b.out["labels"], batches[i]["label"])
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        gs_b(batches[0])
    for la, lb in zip(losses_a, losses_b):
        assert torch.equal(la, lb)
    for (na, pa), (nb, pb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert na == nb and torch.equal(pa, pb), na
    assert (feed.epoch, feed.step) == (0, 4) and not cache.bad_index_seen()


def test_staged_graphs_fetch_in_the_first_graph():
    """collectives='staged' at one RCCL rank: the fetch is captured with the forward in graph 0,
    so each call's four stage graphs train on the feed's next batch -- same losses and
    parameters as the staged step handed those batches."""
    import torch.distributed as dist
    from multimodal_alzheimer_amd.data_parallel import GradAllReduce
    from multimodal_alzheimer_amd.graph_step import GraphedTrainStep, backward_stages
    g = torch.Generator().manual_seed(10)
    n, s, bs, warm = 6, 32, 2, 1
    x = torch.rand((n, s, s, s), dtype=torch.float32, generator=g).double()
    y = torch.randint(0, 2, (n,), generator=g)
    cache = dc.DeviceVolumeCache.from_tensors(y, mri=x)
    assert cache.storage == "float32"
    feed = cache.feed(bs, shuffle=True, seed=6)
    batches = [cache.fetch(i) for i in feed.epoch_batches(0)]
    torch.manual_seed(17)
    a = M.Anat_CNN(_hparams()).cuda()
    b = copy.deepcopy(a)
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:29577", rank=0, world_size=1,
                            device_id=torch.device("cuda", torch.cuda.current_device()))
    try:
        losses = []
        for m, fd in ((a, None), (b, feed)):
            red = GradAllReduce(m.parameters(), bucket_mb=None, stages=backward_stages(m)[1])
            gs = GraphedTrainStep(m, m.configure_optimizers(), batches[0], warmup=warm,
                                  reducer=red, collectives="staged", feed=fd)
            assert len(gs.graphs) == 4
            losses.append([(gs() if fd else gs(batches[i]))["loss"].clone() for i in range(3)])
        torch.cuda.synchronize()
    finally:
        dist.destroy_process_group()
    for la, lb in zip(*losses):
        assert torch.equal(la, lb)
    for (na, pa), (nb, pb) in zip(a.state_dict().items(), b.state_dict().items()):
        assert torch.equal(pa, pb), na
    assert not cache.bad_index_seen()

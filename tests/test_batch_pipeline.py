"""lfm_amd/batch_pipeline.py: the order in which ``run_in_flight`` produces and consumes, the JPEG sink's files, the two naming rules, and -- on the GPU -- that
a batch's result is complete when its consumer reads it on another stream than the lane's."""
from argparse import Namespace

import pytest
import torch

from lfm_amd import batch_pipeline as bp
from lfm_amd import io_formats


def _logged(lanes, n_batches, depth=None):
    log, seen, got = [], [], []

    def produce(i, model, vae):
        log.append(f"p{i}")
        seen.append((model, vae))
        return ("item", i)

    def consume(index, item):
        log.append(f"c{index}")
        got.append((index, item))

    bp.run_in_flight(lanes, n_batches, produce, consume, **({} if depth is None else {"depth": depth}))
    return " ".join(log), seen, got


def test_two_lanes_five_batches_default_depth():
    lanes = [("m0", "v0", None), ("m1", "v1", None)]
    log, seen, got = _logged(lanes, 5)
    assert log == "p0 p1 p2 c0 p3 c1 p4 c2 c3 c4"
    assert seen == [(f"m{i % 2}", f"v{i % 2}") for i in range(5)]
    assert got == [(i, ("item", i)) for i in range(5)]


def test_one_lane_three_batches_at_depth_1_and_0():
    lanes = [("m", "v", None)]
    assert _logged(lanes, 3, depth=1)[0] == "p0 p1 c0 p2 c1 c2"
    assert _logged(lanes, 3, depth=0)[0] == "p0 c0 p1 c1 p2 c2"
    assert _logged(lanes, 0) == ("", [], []) == _logged(lanes, 0, depth=0)


def test_host_sink_files_and_the_naming_rules(tmp_path):
    import jpeg_cases as jc
    import numpy as np

    imgs = torch.from_numpy(np.stack([jc.make_image(f, 17, 31)[0] for f in ("blur", "noise")]))  # the case of tests/test_jpeg_ref.py
    sink = bp.JpegSink("host", str(tmp_path / "sink"), world_size=4, rank=1)
    sink.finish(sink.begin(imgs), 6)
    io_formats.save_indexed_jpegs(imgs, str(tmp_path / "ref"), 6, world_size=4, rank=1)
    assert sorted(p.name for p in (tmp_path / "sink").iterdir()) == ["11.jpg", "7.jpg"]
    for nm in ("7.jpg", "11.jpg"):
        assert (tmp_path / "sink" / nm).read_bytes() == (tmp_path / "ref" / nm).read_bytes()
    with pytest.raises(ValueError, match="host or device"):
        bp.JpegSink("gpu", str(tmp_path))

    args = Namespace(save_dir=None, dataset="celeba_256", exp="celeb_f8_dit", epoch_id=475, method="dopri5", use_karras_samplers=False, atol=1e-5, rtol=1e-5,
                     num_steps=40, num_classes=None, cfg_scale=1.0)
    assert bp.default_save_dir(args) == "./generated_samples/celeba_256/expceleb_f8_dit_ep475_mdopri5"
    assert bp.sheet_path(args) == "./samples_celeba_256_dopri5_1e-05_1e-05.jpg"
    args.use_karras_samplers, args.method, args.num_steps, args.num_classes, args.cfg_scale = True, "heun", 5, 10, 1.5
    assert bp.sheet_path(args) == "./samples_celeba_256_heun_5_cfg1.5.jpg"
    args.num_classes = 1  # one class is no guidance suffix
    assert bp.sheet_path(args) == "./samples_celeba_256_heun_5.jpg"
    args.use_karras_samplers, args.method, args.num_classes, args.save_dir = False, "euler", 1000, "out/dir"
    assert bp.sheet_path(args) == "out/dir/samples_celeba_256_euler_1e-05_1e-05_cfg1.5.jpg"
    assert bp.default_save_dir(args) == "out/dir"


@pytest.mark.gpu
def test_consume_sees_the_finished_batch_of_a_lane_stream():
    """Two lane streams, four batches: produce runs inside its lane's stream and leaves a fill and a dependent add of 1 Mi elements enqueued there; consume runs
    on the default stream, after the lane's event, and finds every element written."""
    dev = torch.device("cuda:0")
    default = torch.cuda.current_stream(dev)
    lanes = [("m0", "v0", torch.cuda.Stream(dev)), ("m1", "v1", torch.cuda.Stream(dev))]
    consumed = []

    def produce(i, model, vae):
        assert (model, vae) == lanes[i % 2][:2] and torch.cuda.current_stream(dev) == lanes[i % 2][2]
        x = torch.empty(1 << 20, dtype=torch.float32, device=dev)
        x.fill_(float(i))
        return x + 1.0

    def consume(index, item):
        assert torch.cuda.current_stream(dev) == default
        host = item.cpu()
        assert bool((host == float(index + 1)).all()), (index, host.unique().tolist()[:8])
        consumed.append(index)

    bp.run_in_flight(lanes, 4, produce, consume)
    bp.join_lanes(lanes, dev)
    assert consumed == [0, 1, 2, 3]

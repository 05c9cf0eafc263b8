"""What the sampling drivers share around their models: the lanes, the loop that keeps batches in flight with the host's work a few batches behind, the JPEG
sink and the two naming rules.  ``test_flow_latent.run_modes`` (and with it the layout and --jpeg_encoder drivers), the two _ddp drivers and the downstream
drivers run on these; a fix to the stream ordering is made here, once.

A lane is ``(model, vae, stream)``: batch i runs on lane i % lanes, inside that lane's stream, and the host takes a batch's result only after the event recorded
behind it on that stream, OUTSIDE the stream context -- inside it, a device-to-host copy queues on the lane stream behind the batch just enqueued and the host
cannot launch the next one (the finding recorded in test_flow_latent_ddp.run)."""
import os
from collections import deque

import torch

from . import io_formats


def make_lanes(model, vae, device, n_lanes):
    """[(model, vae, stream)] x n_lanes for batches in flight on one GPU: lane 0 is the model itself, the others are concurrency twins (same packed weights, own
    workspace / solver buffers / captured graphs).  Every lane stream first waits for the stream the weights were loaded and packed on.  Batches of a sampling job
    are independent (reference test_flow_latent_ddp.py:128-146) and a lane's result is bit-identical to the one-lane result (tests/test_gpu_cosched.py)."""
    from .solvers import concurrency_twin

    cur = torch.cuda.current_stream(device)
    lanes = []
    for k in range(max(1, n_lanes)):
        st = torch.cuda.Stream(device)
        st.wait_stream(cur)
        lanes.append((model if k == 0 else concurrency_twin(model), vae if k == 0 or vae is None else concurrency_twin(vae), st))
    return lanes


def lanes_for(args, model, vae, device):
    """--in_flight -> lanes: 0 means 2 on a GPU and 1 on the CPU.  More than one lane on a GPU is ``make_lanes``; one lane is the model itself on the current
    stream, or on no stream at all (None) on a CPU device (the gloo rehearsal of the _ddp driver)."""
    on_gpu = torch.device(device).type == "cuda"
    n_lanes = int(getattr(args, "in_flight", 0) or 0) or (2 if on_gpu else 1)
    if n_lanes > 1 and on_gpu:
        return make_lanes(model, vae, device, n_lanes)
    return [(model, vae, torch.cuda.current_stream(device) if on_gpu else None)]


def join_lanes(lanes, device):
    """The current stream waits for every lane: what the caller enqueues next (a barrier, the next job) is ordered behind the lanes' last batches."""
    for _, _, st in lanes:
        if st is not None:
            torch.cuda.current_stream(device).wait_stream(st)


def run_in_flight(lanes, n_batches, produce, consume, depth=None):
    """Batch i: ``produce(i, model, vae)`` inside lane i % lanes' stream, an event behind it; then, while more than `depth` batches are pending, the oldest one's
    event is awaited and ``consume(index, item)`` gets what its produce returned; after the last batch the rest, in order.  depth = lanes (the default) keeps
    every lane busy under the host's work, depth = 0 consumes each batch right behind its produce.  produce runs in batch order on the calling thread (noise and
    labels come from one generator in that order), consume outside any lane's stream context.  A lane without a stream (None) has no context and no event."""
    depth = len(lanes) if depth is None else depth
    pending = deque()

    def drain():
        done, item, index = pending.popleft()
        if done is not None:
            done.synchronize()
        consume(index, item)

    for i in range(n_batches):
        model, vae, st = lanes[i % len(lanes)]
        if st is None:
            pending.append((None, produce(i, model, vae), i))
        else:
            with torch.cuda.stream(st):
                item = produce(i, model, vae)
                done = torch.cuda.Event()
                done.record(st)
            pending.append((done, item, i))
        while len(pending) > depth:
            drain()
    while pending:
        drain()


class JpegSink:
    """One uint8 NHWC batch -> its indexed JPEG files (``j * world_size + rank + start``.jpg), by either encoder: ``begin`` inside produce, ``finish`` inside
    consume.  "host": begin keeps the tensor, finish copies the pixels and encodes with PIL.Image.save.  "device": begin enqueues the HIP encoder on the current
    stream, finish fetches the lengths and the compressed bytes and writes them -- the same bytes in the same files."""

    def __init__(self, encoder, save_dir, world_size=1, rank=0):
        if encoder not in ("host", "device"):
            raise ValueError(f"jpeg encoder must be host or device, got {encoder!r}")
        self.on_device, self.save_dir, self.world_size, self.rank = encoder == "device", save_dir, world_size, rank

    def begin(self, u8):
        return io_formats.begin_jpegs_device(u8) if self.on_device else u8

    def finish(self, job, start):
        if self.on_device:
            io_formats.write_indexed_files(io_formats.finish_jpegs_device(job), self.save_dir, start, world_size=self.world_size, rank=self.rank)
        else:
            io_formats.save_indexed_jpegs(job.cpu(), self.save_dir, start, world_size=self.world_size, rank=self.rank)


def default_save_dir(args):
    """--save_dir, or the reference's directory of per-image samples (test_flow_latent.py:257, _ddp:113)."""
    return args.save_dir or "./generated_samples/{}/exp{}_ep{}_m{}".format(args.dataset, args.exp, args.epoch_id, args.method)


def sheet_path(args):
    """The default mode's one sample sheet, named as the reference names it (test_flow_latent.py:288-298), under --save_dir when that is given."""
    if not args.use_karras_samplers:
        path = "./samples_{}_{}_{}_{}".format(args.dataset, args.method, args.atol, args.rtol)
    else:
        path = "./samples_{}_{}_{}".format(args.dataset, args.method, args.num_steps)
    if args.num_classes is not None and args.num_classes > 1:
        path += "_cfg{}".format(args.cfg_scale)
    return (os.path.join(args.save_dir, os.path.basename(path)) if args.save_dir else path) + ".jpg"

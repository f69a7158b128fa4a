"""The step before the hot path: preprocessed scene files -> NaN-padded batch dicts on the
GPU, sharded over the data-parallel ranks.

Mirrors the pieces of OpenSceneFlow's ``src/dataset.py`` the reference's ``train.py`` wires into its DataLoader
([REF assets/slurm/1_train.sh:16-30]: node-local staging, ``train_data=<dir> num_workers=16``; the module itself is in the
absent submodule, so names and semantics are recalled):

* ``HDF5Dataset(directory)``: ``index_total.pkl`` = [[scene_id, timestamp], ...]; item = sweep + the next sweep of the same
  scene: ``pc0 gm0 pose0 pc1 gm1 pose1`` and, when labelled, ``flow flow_is_valid flow_category_indices ego_motion``.
  Files are read with the in-tree HDF5 reader (``h5scene.py``; h5py is not in this image).
* ``collate_fn_pad``: drops ground points, pads every cloud of the batch to the longest with NaN rows (the padding the
  voxeliser drops again [REF deflow.py:51-52,82-83]); ``flow`` is padded alike, masks / classes with 0.
* ``ShardedSampler``: torch ``DistributedSampler`` semantics (seeded per-epoch shuffle, padded to a multiple of the world
  size, rank r takes indices r, r + world, ...), no torch.distributed dependency.
* ``SceneLoader``: worker processes (torch DataLoader) read and collate ahead of the training loop; batches go
  host-pinned -> HBM on a copy stream and are handed over with an event, so the H2D traffic (2 clouds x ~1 MB per pair)
  overlaps the previous step.
* ``stage_to_local``: the parallel copy of the scene files to node-local scratch that ``1_train.sh`` does with xargs.
"""
from __future__ import annotations

import os
import pickle
import shutil
import threading
from collections import OrderedDict
from concurrent.futures import ThreadPoolExecutor
from typing import Dict, Iterator, List, Optional, Sequence

import torch

from .h5scene import H5File
from .odometry import check_pose_source, load_pose_sidecar, sweep_pose


class HDF5Dataset:
    def __init__(self, directory: str, max_open_files: int = 8, eval: bool = False, dynamic_key: str = "dufo_label",
                 dynamic_sidecar: Optional[str] = ".dufo.npz", ground_sidecar: str = ".ground.npz", ground_source: str = "auto",
                 flow_sidecar: Optional[str] = None, pose_source: str = "auto", pose_sidecar: Optional[str] = ".pose.npz"):
        """``dynamic_key``: the per-sweep dataset holding the per-point dynamic flag (non-zero = dynamic) that online cluster labels
        start from (``Trainer(cluster_labels=...)``).  UNPINNED: ``dufo_label`` is the name recalled from upstream's process.py (the
        DUFO pass writes it before HDBSCAN turns it into ``label``), hence an argument.  When both sweeps of a pair hold it, the item
        carries ``dufo0`` / ``dufo1``; files without it give the items they always gave.
        ``dynamic_sidecar``: when a pair's groups lack ``dynamic_key`` and ``<directory>/<scene_id><dynamic_sidecar>`` exists -- the file
        ``python -m deflow_amd.voidmap data_dir=<directory>`` writes: one 0 / 1 array per timestamp, computed on the GPU by the void map
        of DESIGN.md section 6c (UNPINNED) -- ``dufo0`` / ``dufo1`` come from it.  An array whose length differs from the sweep's rows
        is a ValueError; a directory without sidecars gives the items it always gave.  None or "" switches the lookup off.
        ``ground_source`` / ``ground_sidecar``: where ``gm0`` / ``gm1`` come from.  "auto": a group's own ``ground_mask`` dataset wins; a
        group without one takes its mask from ``<directory>/<scene_id><ground_sidecar>`` -- the file
        ``python -m deflow_amd.ground data_dir=<directory>`` writes: one 0 / 1 array per timestamp, computed on the GPU by the ground
        segmenter of DESIGN.md section 6d (UNPINNED) -- and when neither exists a KeyError names that command.  "file": the dataset only.
        "sidecar": the sidecar only, which must exist; the datasets are ignored.  An array whose length differs from the sweep's rows is
        a ValueError.  A directory whose files carry ``ground_mask`` gives the items it always gave.
        ``flow_sidecar``: a ``res_name``.  A pair whose first group holds no ``flow`` dataset takes ``flow`` from
        ``<directory>/<scene_id>.<res_name>.flow.npz`` -- the file ``python -m deflow_amd.save`` writes: the total flow of every raw row
        per timestamp (pseudo labels, e.g. of ``save model=icpflow``) -- with ``flow_is_valid`` all true and
        ``flow_category_indices`` all zero.  A missing file or timestamp is a KeyError naming that command, an array whose length differs
        from the sweep's rows a ValueError.  A group that has ``flow`` keeps it.  None: the items the directory always gave.
        ``pose_source`` / ``pose_sidecar``: where ``pose0`` / ``pose1`` come from, like ``ground_source``.  "auto": a group's own ``pose``
        dataset wins (every file that holds one gives the items it always gave); a group without one takes its pose from
        ``<directory>/<scene_id><pose_sidecar>`` -- the file ``python -m deflow_amd.odometry data_dir=<directory>`` writes: one float64
        [4,4] per timestamp, registered on the GPU by the odometry of DESIGN.md section 6r (UNPINNED).  "file": the dataset only.
        "sidecar": the sidecar only, which must exist.  A sidecar that is missing or lacks a timestamp is a ValueError naming that command.
        ``eval=True`` (the evaluation entry): read ``index_eval.pkl`` -- the frames of the official validation benchmark, the ones
        that carry an ``eval_mask`` -- when the directory has one, as upstream's dataset does for ``av2_mode=val`` (recalled: the
        module is in the absent submodule); ``index_total.pkl`` lists every sweep of every scene."""
        self.directory = directory
        self.dynamic_key = dynamic_key
        self.dynamic_sidecar = dynamic_sidecar
        if ground_source not in ("auto", "file", "sidecar"):
            raise ValueError(f"ground_source must be 'auto', 'file' or 'sidecar', got {ground_source!r}")
        if ground_source == "sidecar" and not ground_sidecar:
            raise ValueError("ground_source='sidecar' needs a ground_sidecar suffix")
        self.ground_sidecar = ground_sidecar
        self.ground_source = ground_source
        if flow_sidecar is not None and (not flow_sidecar or os.sep in str(flow_sidecar)):
            raise ValueError(f"flow_sidecar must be the res_name of a flow file, got {flow_sidecar!r}")
        self.flow_sidecar = flow_sidecar
        check_pose_source(pose_source, pose_sidecar)
        self.pose_source, self.pose_sidecar = pose_source, pose_sidecar
        self._pose_sidecars: "OrderedDict[str, Optional[dict]]" = OrderedDict()
        self._flow_sidecars: "OrderedDict[str, Optional[dict]]" = OrderedDict()
        self._sidecars: "OrderedDict[str, Optional[dict]]" = OrderedDict()       # cached per scene like the open files (None: no file)
        self._ground_sidecars: "OrderedDict[str, Optional[dict]]" = OrderedDict()
        name = "index_total.pkl"
        if eval and os.path.exists(os.path.join(directory, "index_eval.pkl")):
            name = "index_eval.pkl"
        self.index_file = name
        with open(os.path.join(directory, name), "rb") as f:
            self.data_index: List[Sequence] = [list(e) for e in pickle.load(f)]
        self._files: "OrderedDict[str, H5File]" = OrderedDict()
        self._lock = threading.Lock()
        self._max_open = max_open_files

    def __len__(self) -> int:
        return len(self.data_index)

    def _file(self, scene_id: str) -> H5File:
        with self._lock:
            f = self._files.get(scene_id)
            if f is None:
                f = H5File(os.path.join(self.directory, f"{scene_id}.h5"))
                f.sweeps = sorted(f.keys(), key=int)          # timestamps in time order
                self._files[scene_id] = f
                while len(self._files) > self._max_open:
                    self._files.popitem(last=False)   # not closed here: a worker may still be reading it; the map is
                                                      # released when the last reference goes
            else:
                self._files.move_to_end(scene_id)
            return f

    def _sidecar(self, scene_id: str, ground: bool = False) -> Optional[dict]:
        cache, suffix = (self._ground_sidecars, self.ground_sidecar) if ground else (self._sidecars, self.dynamic_sidecar)
        with self._lock:
            if scene_id in cache:
                cache.move_to_end(scene_id)
                return cache[scene_id]
        path = os.path.join(self.directory, f"{scene_id}{suffix}")
        side = None
        if os.path.exists(path):
            import numpy as np
            with np.load(path, allow_pickle=False) as z:
                side = {k: z[k] for k in z.files if k != "meta"}
        with self._lock:
            cache[scene_id] = side
            while len(cache) > self._max_open:
                cache.popitem(last=False)
        return side

    def _pseudo_flow(self, scene_id: str, ts: str, rows: int) -> torch.Tensor:
        """the flow of one sweep's raw rows from ``<scene_id>.<flow_sidecar>.flow.npz``"""
        name = f"{scene_id}.{self.flow_sidecar}.flow.npz"
        with self._lock:
            known = scene_id in self._flow_sidecars
            side = self._flow_sidecars.get(scene_id)
        if not known:
            path = os.path.join(self.directory, name)
            if os.path.exists(path):
                import numpy as np
                with np.load(path, allow_pickle=False) as z:
                    side = {k: z[k] for k in z.files if k != "meta" and not k.endswith(".dynamic")}
            with self._lock:
                self._flow_sidecars[scene_id] = side
                while len(self._flow_sidecars) > self._max_open:
                    self._flow_sidecars.popitem(last=False)
        if side is None or ts not in side:
            what = "does not exist" if side is None else f"has no entry for sweep {ts}"
            raise KeyError(f"{scene_id}: sweep {ts} has no flow dataset and {name} {what}; write it with  python -m deflow_amd.save "
                           f"dataset_path={self.directory} res_name={self.flow_sidecar} (model=icpflow needs no checkpoint)")
        flow = torch.from_numpy(side[ts])
        if flow.dim() != 2 or flow.shape[1] != 3 or flow.shape[0] != rows:
            raise ValueError(f"{name}: flow of shape {tuple(flow.shape)} for sweep {ts}, which has {rows} rows: the file belongs to "
                             "another version of the scene file")
        return flow.float()

    def _pose(self, scene_id: str, ts: str, group) -> torch.Tensor:
        """the pose of one sweep, by ``pose_source``"""
        source = getattr(self, "pose_source", "auto")
        if source == "file" or (source == "auto" and "pose" in group):
            return torch.from_numpy(group["pose"].read())
        with self._lock:
            known = scene_id in self._pose_sidecars
            side = self._pose_sidecars.get(scene_id)
        if not known:
            side = load_pose_sidecar(self.directory, scene_id, self.pose_sidecar)
            with self._lock:
                self._pose_sidecars[scene_id] = side
                while len(self._pose_sidecars) > self._max_open:
                    self._pose_sidecars.popitem(last=False)
        return torch.from_numpy(sweep_pose(group, side, scene_id=scene_id, ts=ts, pose_source=source, pose_sidecar=self.pose_sidecar,
                                           directory=self.directory))

    def _ground(self, scene_id: str, ts: str, group, rows: int) -> torch.Tensor:
        """the ground mask of one sweep, by ``ground_source``"""
        if self.ground_source == "file" or (self.ground_source == "auto" and "ground_mask" in group):
            return torch.from_numpy(group["ground_mask"].read())
        side = self._sidecar(scene_id, ground=True) if self.ground_sidecar else None
        if side is None or ts not in side:
            what = "does not exist" if side is None else f"has no entry for sweep {ts}"
            raise KeyError(f"{scene_id}: no ground mask for sweep {ts} (ground_source={self.ground_source!r}): "
                           f"{scene_id}{self.ground_sidecar} {what}; write it with  python -m deflow_amd.ground data_dir={self.directory}")
        mask = torch.from_numpy(side[ts]).reshape(-1)
        if mask.shape[0] != rows:
            raise ValueError(f"{scene_id}{self.ground_sidecar}: {mask.shape[0]} ground flags for sweep {ts}, which has {rows} rows: "
                             "the sidecar belongs to another version of the scene file")
        return mask != 0

    def __getitem__(self, index: int) -> Dict[str, object]:
        scene_id, timestamp = self.data_index[index][0], str(self.data_index[index][1])
        f = self._file(scene_id)
        k = f.sweeps.index(timestamp)
        if k + 1 >= len(f.sweeps):
            # upstream's index (create_reading_index) lists EVERY sweep of a scene; the last one has no successor, and
            # upstream's HDF5Dataset steps such an entry back by one sweep instead of failing
            if len(f.sweeps) < 2:
                raise IndexError(f"{scene_id} holds a single sweep: nothing to pair {timestamp} with")
            k -= 1
            timestamp = f.sweeps[k]
        g0, g1 = f[timestamp], f[f.sweeps[k + 1]]
        t = lambda d: torch.from_numpy(d.read())
        pc0, pc1 = t(g0["lidar"])[:, :3], t(g1["lidar"])[:, :3]
        item = {"scene_id": scene_id, "timestamp": int(timestamp),
                "pc0": pc0, "gm0": self._ground(scene_id, timestamp, g0, pc0.shape[0]), "pose0": self._pose(scene_id, timestamp, g0),
                "pc1": pc1, "gm1": self._ground(scene_id, f.sweeps[k + 1], g1, pc1.shape[0]), "pose1": self._pose(scene_id, f.sweeps[k + 1], g1)}
        if "flow" in g0:
            item.update(flow=t(g0["flow"]), flow_is_valid=t(g0["flow_is_valid"]),
                        flow_category_indices=t(g0["flow_category_indices"]))
        elif getattr(self, "flow_sidecar", None):      # pseudo labels: every row valid, no classes
            n = int(pc0.shape[0])
            item.update(flow=self._pseudo_flow(scene_id, timestamp, n), flow_is_valid=torch.ones(n, dtype=torch.bool),
                        flow_category_indices=torch.zeros(n, dtype=torch.uint8))
        if "ego_motion" in g0:
            item["ego_motion"] = t(g0["ego_motion"])
        if "label" in g0 and "label" in g1:      # cluster labels of the self-supervised mode (upstream's process.py: DUFO + HDBSCAN; 0 = static)
            item["label0"] = t(g0["label"]).reshape(-1).long()
            item["label1"] = t(g1["label"]).reshape(-1).long()
        dk = self.dynamic_key
        if dk and dk in g0 and dk in g1:         # per-point dynamic flags: the input of the online cluster labels (cluster.py)
            item["dufo0"] = t(g0[dk]).reshape(-1) != 0
            item["dufo1"] = t(g1[dk]).reshape(-1) != 0
        elif self.dynamic_sidecar:
            side = self._sidecar(scene_id)
            t1 = f.sweeps[k + 1]
            if side is not None and timestamp in side and t1 in side:
                for key, ts, pc in (("dufo0", timestamp, "pc0"), ("dufo1", t1, "pc1")):
                    flags = torch.from_numpy(side[ts]).reshape(-1)
                    if flags.shape[0] != item[pc].shape[0]:
                        raise ValueError(f"{scene_id}{self.dynamic_sidecar}: {flags.shape[0]} flags for sweep {ts}, which has "
                                         f"{item[pc].shape[0]} rows: the sidecar belongs to another version of the scene file")
                    item[key] = flags != 0
        if "eval_mask" in g0:          # the benchmark's point mask of the official validation split
            item["eval_mask"] = t(g0["eval_mask"]).reshape(-1).bool()
        return item


def _pad(seqs: List[torch.Tensor], value) -> torch.Tensor:
    n = max(int(s.shape[0]) for s in seqs)
    out = seqs[0].new_full((len(seqs), n) + tuple(seqs[0].shape[1:]), value)
    for i, s in enumerate(seqs):
        out[i, : s.shape[0]] = s
    return out


def collate_fn_pad(batch: List[Dict[str, object]]) -> Dict[str, object]:
    keep0 = [~b["gm0"] for b in batch]
    keep1 = [~b["gm1"] for b in batch]
    res: Dict[str, object] = {
        "pc0": _pad([b["pc0"][k].float() for b, k in zip(batch, keep0)], float("nan")),
        "pc1": _pad([b["pc1"][k].float() for b, k in zip(batch, keep1)], float("nan")),
        "pose0": torch.stack([b["pose0"].float() for b in batch]),
        "pose1": torch.stack([b["pose1"].float() for b in batch]),
        "scene_id": [b["scene_id"] for b in batch], "timestamp": [b["timestamp"] for b in batch],
    }
    if "flow" in batch[0]:
        res["flow"] = _pad([b["flow"][k].float() for b, k in zip(batch, keep0)], float("nan"))
        res["flow_is_valid"] = _pad([b["flow_is_valid"][k] for b, k in zip(batch, keep0)], False)
        res["flow_category_indices"] = _pad([b["flow_category_indices"][k] for b, k in zip(batch, keep0)], 0)
    if all("label0" in b and "label1" in b for b in batch):
        # seflowLoss's batch keys (upstream's names, recalled): ground rows dropped like the points, padded rows 0; max_label (a Python
        # int, known here for free) sizes the loss's per-label tables without a device read-back
        res["pc0_dynamic"] = _pad([b["label0"][k].long() for b, k in zip(batch, keep0)], 0)
        res["pc1_dynamic"] = _pad([b["label1"][k].long() for b, k in zip(batch, keep1)], 0)
        res["max_label"] = int(max(int(res["pc0_dynamic"].max()), int(res["pc1_dynamic"].max()), 0))
    if all("dufo0" in b and "dufo1" in b for b in batch):
        # dynamic flags for Trainer(cluster_labels=...): ground rows dropped and padded rows 0, exactly like the labels
        res["pc0_dufo"] = _pad([(b["dufo0"][k] != 0).long() for b, k in zip(batch, keep0)], 0)
        res["pc1_dufo"] = _pad([(b["dufo1"][k] != 0).long() for b, k in zip(batch, keep1)], 0)
    if "ego_motion" in batch[0]:
        res["ego_motion"] = torch.stack([b["ego_motion"].float() for b in batch])
    if any("eval_mask" in b for b in batch):
        # per SAMPLE: upstream's preprocessing writes the mask on the official evaluation frames only, so a batch of the
        # validation split mixes frames with and without one.  A frame without a mask gets an all-True one (every valid point
        # counts) and has_eval_mask = False, which lets the evaluation skip it where the benchmark would.
        res["eval_mask"] = _pad([(b["eval_mask"][k] if "eval_mask" in b else torch.ones(int(k.sum()), dtype=torch.bool))
                                 for b, k in zip(batch, keep0)], False)
        res["has_eval_mask"] = torch.tensor(["eval_mask" in b for b in batch], dtype=torch.bool)
    return res


class ShardedSampler:
    def __init__(self, n: int, rank: int = 0, world: int = 1, shuffle: bool = True, seed: int = 0, drop_last: bool = False):
        self.n, self.rank, self.world, self.shuffle, self.seed, self.epoch = n, rank, world, shuffle, seed, 0
        self.num_samples = n // world if drop_last else (n + world - 1) // world
        self.total = self.num_samples * world

    def set_epoch(self, epoch: int):
        self.epoch = epoch

    def __len__(self) -> int:
        return self.num_samples

    def __iter__(self) -> Iterator[int]:
        if self.shuffle:
            g = torch.Generator()
            g.manual_seed(self.seed + self.epoch)
            idx = torch.randperm(self.n, generator=g).tolist()
        else:
            idx = list(range(self.n))
        if len(idx) < self.total:                     # pad by wrapping around, as DistributedSampler does
            idx += (idx * ((self.total - len(idx)) // max(len(idx), 1) + 1))[: self.total - len(idx)]
        return iter(idx[: self.total][self.rank: self.total: self.world])


class SceneLoader:
    """for batch in SceneLoader(...): batch tensors are on `device`, ready on the current stream.

    Reading and collating run in `num_workers` worker PROCESSES (torch DataLoader, as in the reference's train.py): the
    training loop launches ~400 kernels per step from Python, and reader threads in the same interpreter starve it through
    the GIL (measured: 44 pairs/s with threads vs the resident-batch rate with processes).  The parent keeps `prefetch`
    batches in flight host-pinned -> HBM on a copy stream and hands each over with an event."""

    def __init__(self, dataset, batch_size: int, sampler: Optional[ShardedSampler] = None, device=None, num_workers: int = 4,
                 prefetch: int = 3, drop_last: bool = True):
        self.ds, self.bs, self.device = dataset, batch_size, device
        self.sampler = sampler or ShardedSampler(len(dataset), shuffle=False)
        self.workers, self.prefetch, self.drop_last = max(0, num_workers), max(1, prefetch), drop_last

    def __len__(self) -> int:
        n = len(self.sampler)
        return n // self.bs if self.drop_last else (n + self.bs - 1) // self.bs

    def __iter__(self):
        from torch.utils.data import DataLoader
        cuda = self.device is not None and torch.device(self.device).type == "cuda"
        if getattr(self, "_dl", None) is None:   # one DataLoader for all epochs: its worker processes persist (a restart
            kw = dict(prefetch_factor=2, persistent_workers=True) if self.workers else {}   # costs seconds per epoch)
            self._dl = DataLoader(self.ds, batch_size=self.bs, sampler=self.sampler, collate_fn=collate_fn_pad,
                                  num_workers=self.workers, pin_memory=cuda, drop_last=self.drop_last, **kw)
        host = iter(self._dl)
        if not cuda:
            yield from host
            return
        copy_stream = torch.cuda.Stream(device=self.device)
        inflight: List = []

        def fetch():
            b = next(host, None)
            if b is None:
                return False
            with torch.cuda.stream(copy_stream):
                dev = {k: (v.to(self.device, non_blocking=True) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            inflight.append((dev, ev, b))          # b: the pinned source stays alive until the copy is consumed
            return True

        while len(inflight) < self.prefetch and fetch():
            pass
        while inflight:
            dev, ev, _ = inflight.pop(0)
            torch.cuda.current_stream().wait_event(ev)
            for v in dev.values():                 # allocated on the copy stream: tie their lifetime to this stream
                if isinstance(v, torch.Tensor):
                    v.record_stream(torch.cuda.current_stream())
            fetch()
            yield dev


def stage_to_local(src: str, dst: str, workers: int = 16) -> int:
    """copy every file under `src` to `dst` (flat, like `find ... | xargs -P16 cp -t` [REF 1_train.sh:16-24]); returns
    the number of bytes copied; files already present with the same size are skipped"""
    os.makedirs(dst, exist_ok=True)
    jobs = []
    for root, _, names in os.walk(src):
        for n in names:
            s, d = os.path.join(root, n), os.path.join(dst, n)
            if not (os.path.exists(d) and os.path.getsize(d) == os.path.getsize(s)):
                jobs.append((s, d))
    with ThreadPoolExecutor(max(1, workers)) as pool:
        list(pool.map(lambda sd: shutil.copyfile(*sd), jobs))
    return sum(os.path.getsize(s) for s, _ in jobs)

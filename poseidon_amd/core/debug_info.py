"""Solver debug_info: per-layer blob statistics of one training step.

The reference's Net::ForwardDebugInfo / BackwardDebugInfo / UpdateDebugInfo
(net.cpp:787-852) print the mean absolute value of every top blob, every
bottom and param diff, and every param's data and update. Here each of those
is one slot of a persistent statistics buffer (ops.BlobStatsBuffer): the
layers' tensors are read in place by the blob-statistics kernels while the
step runs -- no host sync, nothing a hipGraph capture cannot record -- and
records() copies the buffer back once.

Slot layout, fixed when the object is made:
    [0, n_fwd)        (layer, top), layer order
    [n_fwd, n_bwd)    (layer, bottom that needs a gradient), layer order,
                      then one per param diff
    [n_bwd, n_all)    per param: data before the update, then the update
The three ranges are the three phases; each is finalized by one launch.

The statistics describe the step that actually runs, fused paths included
(docs/architecture.md, "debug_info"): records carry a note where that
departs from the reference's unfused value, and available=False where a
fused kernel never materializes the tensor.
"""

from __future__ import annotations

from typing import Dict, List, Optional

import torch

from .context import ctx
from ..ops import functional as ops


class DebugInfo:
    def __init__(self, net) -> None:
        self.net = net
        n = 0
        self.top_slot: List[List[int]] = []
        for tops in net.tops:
            self.top_slot.append(list(range(n, n + len(tops))))
            n += len(tops)
        self.n_fwd = n
        self.bottom_slot: List[List[Optional[int]]] = []
        for i, need in enumerate(net.bottom_need_bwd):
            row: List[Optional[int]] = []
            for nb in need:
                if nb and net.layer_need_bwd[i]:
                    row.append(n)
                    n += 1
                else:
                    row.append(None)
            self.bottom_slot.append(row)
        np_ = len(net.params)
        self.pdiff_slot = list(range(n, n + np_))
        n += np_
        self.n_bwd = n
        self.pdata_slot = list(range(n, n + np_))
        self.pupd_slot = list(range(n + np_, n + 2 * np_))
        self.n_all = n + 2 * np_
        self.buf = ops.BlobStatsBuffer(self.n_all, ctx().torch_device)
        self._count: Dict[int, int] = {}
        self._avail: Dict[int, bool] = {}
        self._ran: set = set()
        self._mt: Dict[str, tuple] = {}

    # -- launches ---------------------------------------------------------
    def _stat(self, t: torch.Tensor, slot: int) -> None:
        """Single-tensor launch: activations, whose identity may change from
        step to step. A view that is not dense is reported unavailable (the
        kernels read storage in place and never copy)."""
        ok = t.numel() > 0 and ops._stats_dense(t)
        self._avail[slot] = ok
        self._count[slot] = t.numel()
        if ok:
            ops.blob_stats(t, self.buf, slot)

    def _stat_mt(self, which: str, tensors, slots) -> None:
        """One launch over an identity-stable set; the table is rebuilt when
        an identity changes."""
        if not tensors:
            return
        key = [id(t) for t in tensors] + list(slots)
        cur = self._mt.get(which)
        if cur is None or cur[1] != key:
            cur = (ops.blob_stats_mt_prepare(tensors, slots), key)
            self._mt[which] = cur
        ops.blob_stats_mt_run(cur[0], self.buf)
        for t, s in zip(tensors, slots):
            self._avail[s] = True
            self._count[s] = t.numel()

    def begin(self) -> None:
        self._ran = set()
        self._avail = {}

    def tops(self, i: int) -> None:
        for t, slot in zip(self.net.tops[i], self.top_slot[i]):
            self._stat(t.data, slot)

    def end_forward(self) -> None:
        ops.blob_stats_finalize(self.buf, 0, self.n_fwd)
        self._ran.add("forward")

    def bottoms(self, i: int) -> None:
        layer = self.net.layers[i]
        for b, slot in zip(self.net.bottoms[i], self.bottom_slot[i]):
            if slot is None:
                continue
            if (getattr(layer, "bwd_fused_into_producer", False)
                    or not b.has_diff()):
                # never written this step: do not read a stale tensor
                self._avail[slot] = False
                self._count[slot] = b.count
            else:
                self._stat(b.diff, slot)

    def param_diffs(self) -> None:
        """All param diffs in one launch, where they are final: after the
        deferred unpacks and the batched column sums (and, distributed,
        after the all-reduce)."""
        net = self.net
        own = [(i, ps) for i, ps in enumerate(net.params)
               if ps.owner == i and ps.blob.has_diff()]
        self._stat_mt("diff", [ps.blob.diff for _, ps in own],
                      [self.pdiff_slot[i] for i, _ in own])
        ops.blob_stats_finalize(self.buf, self.n_fwd, self.n_bwd - self.n_fwd)
        self._ran.add("backward")

    def update_data(self) -> None:
        """Param data, before the update writes it."""
        own = [(i, ps) for i, ps in enumerate(self.net.params)
               if ps.owner == i]
        self._stat_mt("data", [ps.blob.data for _, ps in own],
                      [self.pdata_slot[i] for i, _ in own])

    def update_values(self, values: Dict[int, torch.Tensor],
                      stable: bool) -> None:
        """values: param index -> the tensor holding its update. stable: the
        tensors keep their identity across steps (SGD's history), so one
        table launch covers them; else one launch each."""
        idx = sorted(values)
        if stable:
            self._stat_mt("update", [values[i] for i in idx],
                          [self.pupd_slot[i] for i in idx])
        else:
            for i in idx:
                self._stat(values[i], self.pupd_slot[i])
        ops.blob_stats_finalize(self.buf, self.n_bwd, self.n_all - self.n_bwd)
        self._ran.add("update")

    # -- read-back --------------------------------------------------------
    def _rec(self, raw, slot: Optional[int], **fields) -> dict:
        ok = slot is not None and self._avail.get(slot, False)
        count = self._count.get(slot, 0) if slot is not None else 0
        asum, maxabs, nf = raw[slot] if ok else (0.0, 0.0, 0)
        fields.update(count=count,
                      mean_abs=float(asum) / count if ok and count else 0.0,
                      max_abs=float(maxabs), nonfinite=int(nf), available=ok)
        fields.setdefault("note", "")
        return fields

    def records(self) -> List[dict]:
        """The last debug pass as a list of records, in the reference's
        print order. One device-to-host copy."""
        net = self.net
        raw = self.buf.records()
        lps = net.param.layers
        out: List[dict] = []
        if "forward" in self._ran:
            for i, layer in enumerate(net.layers):
                for ti, slot in enumerate(self.top_slot[i]):
                    if slot not in self._avail:
                        continue  # partial forward
                    note = ("post-relu" if getattr(layer, "fuse_relu", False)
                            else "")
                    out.append(self._rec(raw, slot, phase="forward",
                                         layer=layer.name, kind="top",
                                         name=lps[i].top[ti], note=note))
        if "backward" in self._ran:
            by_layer: Dict[int, List[int]] = {}
            for idx, ps in enumerate(net.params):
                by_layer.setdefault(ps.layer_idx, []).append(idx)
            for i in range(len(net.layers) - 1, -1, -1):
                if not net.layer_need_bwd[i]:
                    continue
                layer = net.layers[i]
                for j, slot in enumerate(self.bottom_slot[i]):
                    if slot is None:
                        continue
                    note = ""
                    if getattr(layer, "bwd_fused_into_producer", False):
                        note = "fused"
                    elif (getattr(layer, "bwd_fused_into_consumer", False)
                          or j in (getattr(layer, "_mask_bottoms", None)
                                   or ())
                          or (layer.type_name in ("LRN", "POOLING")
                              and getattr(layer, "_tail_conv", None)
                              is not None)):
                        note = "masked"
                    out.append(self._rec(raw, slot, phase="backward",
                                         layer=layer.name, kind="bottom",
                                         name=lps[i].bottom[j], note=note))
                for idx in by_layer.get(i, []):
                    ps = net.params[idx]
                    if ps.lr_mult == 0.0:
                        continue
                    out.append(self._rec(raw, self.pdiff_slot[ps.owner],
                                         phase="backward", layer=layer.name,
                                         kind="param",
                                         param_idx=ps.param_idx))
        if "update" in self._ran:
            for idx, ps in enumerate(net.params):
                own = net.params[ps.owner]
                rec = self._rec(raw, self.pupd_slot[ps.owner],
                                phase="update",
                                layer=net.layers[ps.layer_idx].name,
                                kind="param", param_idx=ps.param_idx,
                                name=ps.name or str(ps.param_idx))
                if own.lr_mult == 0.0:  # frozen: the update is zero
                    rec.update(available=True, count=own.blob.count,
                               note="frozen")
                rec["owner"] = None
                if ps.owner != idx:
                    rec["owner"] = (net.layers[own.layer_idx].name,
                                    own.name or str(own.param_idx))
                else:
                    d = self._rec(raw, self.pdata_slot[idx])
                    rec.update(data_mean_abs=d["mean_abs"],
                               data_max_abs=d["max_abs"],
                               data_nonfinite=d["nonfinite"])
                out.append(rec)
        return out


def _g(v: float) -> str:
    """A value as the reference's ostream prints it: six significant
    digits."""
    return "%g" % v


def format_records(records: List[dict]) -> List[str]:
    """The reference's log lines for these records (net.cpp:787-852), then
    one [Watch] line per record that holds NaN or Inf elements."""
    lines: List[str] = []
    for r in records:
        if r["phase"] == "forward":
            lines.append(f"    [Forward] Layer {r['layer']}, top blob "
                         f"{r['name']} data: {_g(r['mean_abs'])}")
        elif r["phase"] == "backward":
            what = (f"bottom blob {r['name']}" if r["kind"] == "bottom"
                    else f"param blob {r['param_idx']}")
            val = _g(r["mean_abs"]) if r["available"] else "n/a (fused)"
            lines.append(f"    [Backward] Layer {r['layer']}, {what} "
                         f"diff: {val}")
        elif r["owner"] is None:
            lines.append(f"    [Update] Layer {r['layer']}, param "
                         f"{r['name']} data: {_g(r['data_mean_abs'])}; "
                         f"diff: {_g(r['mean_abs'])}")
        else:
            lines.append(f"    [Update] Layer {r['layer']}, param blob "
                         f"{r['name']} (owned by layer {r['owner'][0]}, "
                         f"param {r['owner'][1]}) diff: "
                         f"{_g(r['mean_abs'])}")
    for r in records:
        if r["nonfinite"] > 0:
            name = r["name"] if "name" in r else r["param_idx"]
            lines.append(f"    [Watch] Layer {r['layer']}, {r['kind']} "
                         f"{name}: {r['nonfinite']} non-finite of "
                         f"{r['count']}, max finite |x| {_g(r['max_abs'])}")
    return lines

"""Net: the layer DAG built from a NetParameter.

Parity with /root/reference/src/caffe/net.cpp (Init walk with in-place
detection and shared-param ownership, FilterNet/StateMeetsRule,
ForwardFromTo/BackwardFromTo, CopyTrainedLayersFrom, ToProto). The InitPS
table walk (net.cpp:253-363) has no analogue: parameters are plain device
tensors, synchronized by RCCL collectives.

Backward accepts a post-layer callback so the distributed solver can launch
per-layer gradient all-reduce on a side HIP stream as soon as a layer's
grads exist -- the stream/event realization of Poseidon's DWBP
(solver.cpp:405-451) without host threads.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, List, Optional

import torch

from .blob import Blob
from .context import ctx
from .insert_splits import insert_splits
from .layer import Layer, create_layer
from ..ops import functional as ops
from ..proto import Message, spec
from ..proto.upgrade import net_needs_upgrade, upgrade_v0_net

TRAIN = spec.ENUMS["Phase"]["TRAIN"]
TEST = spec.ENUMS["Phase"]["TEST"]


def state_meets_rule(state: Message, rule: Message) -> bool:
    """NetStateRule check (net.cpp:423-468)."""
    if rule.has("phase") and rule.phase != state.phase:
        return False
    if rule.has("min_level") and state.level < rule.min_level:
        return False
    if rule.has("max_level") and state.level > rule.max_level:
        return False
    stages = set(state.stage)
    for s in rule.stage:
        if s not in stages:
            return False
    for s in rule.not_stage:
        if s in stages:
            return False
    return True


def filter_net(param: Message, state: Message) -> Message:
    out = Message("NetParameter")
    for name in ("name", "input", "input_dim", "force_backward"):
        if param.has(name):
            v = getattr(param, name)
            if name in ("input", "input_dim"):
                getattr(out, name).extend(v)
            else:
                setattr(out, name, v)
    for layer in param.layers:
        inc, exc = list(layer.include), list(layer.exclude)
        if inc and exc:
            raise ValueError(f"layer {layer.name}: specify include OR exclude, not both")
        keep = (any(state_meets_rule(state, r) for r in inc) if inc
                else not any(state_meets_rule(state, r) for r in exc))
        if keep:
            out.layers.append(layer)
    return out


@dataclass
class ParamSpec:
    blob: Blob
    layer_idx: int
    param_idx: int
    lr_mult: float
    decay_mult: float
    owner: int  # index into net.params of the owner (== own index if owner)
    name: str = ""


class Net:
    def __init__(self, param: Message, phase: int = TRAIN,
                 state: Optional[Message] = None, verbose: Optional[bool] = None):
        st = Message("NetState", phase=phase)
        if param.has("state"):
            st.merge_from(param.state)
            st.phase = phase
        if state is not None:
            st.merge_from(state)
        self.phase = phase
        if net_needs_upgrade(param):
            param = upgrade_v0_net(param)  # legacy V0 prototxt support
        filtered = filter_net(param, st)
        self.param = insert_splits(filtered)
        self.name = self.param.name or ""
        self._verbose = ctx().is_root() if verbose is None else verbose

        self.layers: List[Layer] = []
        self.layer_names: List[str] = []
        self.bottoms: List[List[Blob]] = []
        self.tops: List[List[Blob]] = []
        self.bottom_need_bwd: List[List[bool]] = []
        self.layer_need_bwd: List[bool] = []
        self.blobs: Dict[str, Blob] = {}
        self.params: List[ParamSpec] = []
        self._param_name_to_idx: Dict[str, int] = {}
        self.output_blob_names: List[str] = []
        self._loss_tops: List = []  # (layer_idx, top_idx, weight)
        self._zero_mt = None  # multi-tensor zero table (GPU, built lazily)
        self._repack_mt = None  # multi-tensor conv-weight repack table
        self._unpack_mt = None  # deferred conv-wgrad unpack table
        self._colsum_mt = None   # deferred bias-colsum table
        self._colsum_prev_key = None
        self._repack_key = None
        self._repack_entries: List = []  # (layer, master, wk, wkT, G, kw_ld, c_ld)
        self._repack_lite = None  # (table without the marked fc shadows, key)
        self._fc_marks = None     # [(layer, master, _version, shadow)]
        self._loss_marks: Dict[int, List] = {}
        # inter-branch stream parallelism (inception-style nets): built by
        # _build_stream_schedule, activated lazily on GPU
        self._lstream: List[int] = []
        self._producers: List[List[int]] = []
        self._consumers: List[List[int]] = []
        self._ms_nstreams = 0
        self._ms_pool = None
        self._fwd_ev = None
        self._bwd_ev = None
        # solver debug_info (core/debug_info.py): off unless asked for; the
        # slots are laid out at first use. A distributed solver defers the
        # param-diff statistics until its all-reduce is done.
        self._dbg = None
        self._dbg_on = False
        self._dbg_defer_param_diffs = False

        self._build()
        self._build_stream_schedule()

    # ------------------------------------------------------------------
    def _build(self) -> None:
        p = self.param
        available = set()
        blob_need: Dict[str, bool] = {}

        # explicit net inputs (deploy-style nets)
        dims = list(p.input_dim)
        for i, name in enumerate(p.input):
            b = Blob(tuple(dims[4 * i:4 * i + 4]), name=name)
            self.blobs[name] = b
            available.add(name)
            blob_need[name] = False

        force_bwd = bool(p.force_backward)

        for li, lp in enumerate(p.layers):
            layer = create_layer(lp, self.phase)
            self.layers.append(layer)
            self.layer_names.append(layer.name)

            bottoms: List[Blob] = []
            bneed: List[bool] = []
            for bname in lp.bottom:
                if bname not in available:
                    raise ValueError(f"layer {layer.name}: unknown bottom {bname!r}")
                bottoms.append(self.blobs[bname])
                bneed.append(blob_need.get(bname, False) or force_bwd)

            tops: List[Blob] = []
            for ti, tname in enumerate(lp.top):
                if ti < len(lp.bottom) and tname == lp.bottom[ti]:
                    tops.append(self.blobs[tname])  # in-place
                else:
                    if tname in self.blobs:
                        raise ValueError(f"duplicate top blob {tname!r}")
                    b = Blob(name=tname)
                    self.blobs[tname] = b
                    tops.append(b)
                    available.add(tname)

            layer.setup(bottoms, tops)

            # loss weights
            weights = list(lp.loss_weight)
            lw = []
            for ti in range(len(tops)):
                w = weights[ti] if ti < len(weights) else layer.auto_loss_weight(ti)
                lw.append(w)
                if w != 0.0:
                    self._loss_tops.append((li, ti, w))
            layer.loss_weights = lw

            # need-backward propagation
            has_lr = any(layer.blobs_lr(i) != 0.0 for i in range(len(layer.blobs)))
            need = (any(bneed) or (has_lr and len(layer.blobs) > 0)
                    or any(w != 0.0 for w in lw)) and len(lp.bottom) > 0
            # data-ish layers (no bottoms) never run backward
            for tname in lp.top:
                blob_need[tname] = blob_need.get(tname, False) or need
            self.layer_need_bwd.append(need)
            self.bottoms.append(bottoms)
            self.tops.append(tops)
            self.bottom_need_bwd.append(bneed)

            # parameter registration (+ sharing by name)
            pnames = list(lp.param)
            share_modes = list(lp.blob_share_mode)
            for pi, pblob in enumerate(layer.blobs):
                pname = pnames[pi] if pi < len(pnames) else ""
                idx = len(self.params)
                if pname and pname in self._param_name_to_idx:
                    owner_idx = self._param_name_to_idx[pname]
                    owner = self.params[owner_idx]
                    mode = share_modes[pi] if pi < len(share_modes) else 0
                    if mode == 0 and owner.blob.shape != pblob.shape:
                        raise ValueError(
                            f"shared param {pname!r}: shape mismatch "
                            f"{owner.blob.shape} vs {pblob.shape} (STRICT)")
                    if mode == 1 and owner.blob.count != pblob.count:
                        raise ValueError(f"shared param {pname!r}: count mismatch")
                    pblob.share_data(owner.blob)
                    pblob.share_diff(owner.blob)
                    self.params.append(ParamSpec(
                        blob=pblob, layer_idx=li, param_idx=pi,
                        lr_mult=layer.blobs_lr(pi),
                        decay_mult=layer.weight_decay_mult(pi),
                        owner=owner_idx, name=pname))
                else:
                    if pname:
                        self._param_name_to_idx[pname] = idx
                    self.params.append(ParamSpec(
                        blob=pblob, layer_idx=li, param_idx=pi,
                        lr_mult=layer.blobs_lr(pi),
                        decay_mult=layer.weight_decay_mult(pi),
                        owner=idx, name=pname))

            for bname in lp.bottom:
                pass  # blobs stay available (split layers made copies already)

        consumed = {b for lp in p.layers for b in lp.bottom}
        self.output_blob_names = [n for n in available if n not in consumed]

        # Prune layers that do not contribute to any loss from backward
        # (Caffe's layer_contributes_loss logic): ACCURACY/ARGMAX heads etc.
        contributing_blobs = set()
        loss_layers = {li for (li, ti, w) in self._loss_tops}
        for li in range(len(p.layers) - 1, -1, -1):
            lp = p.layers[li]
            contributes = li in loss_layers or any(
                t in contributing_blobs for t in lp.top)
            if contributes:
                contributing_blobs.update(lp.bottom)
            else:
                self.layer_need_bwd[li] = False

        self._fuse_relu_epilogues()
        self._fuse_relu_bwd_into_concats()
        self._fuse_bwd_tails()
        for (li, ti, w) in self._loss_tops:
            self._loss_marks.setdefault(li, []).append((ti, w))
        # Loss layers whose loss top feeds NO consumer get the seeded weight
        # as a host scalar: their backward then never reads top.diff from
        # the device (a D2H sync per iteration that also aborts hipGraph
        # capture). Loss tops that ARE consumed downstream keep the device
        # read (extra gradient may accumulate into the diff).
        for (li, ti, w) in self._loss_tops:
            tname = p.layers[li].top[ti] if ti < len(p.layers[li].top) else None
            if tname is not None and tname not in consumed:
                self.layers[li].seeded_loss_weight = w

    def _fuse_relu_bwd_into_concats(self) -> None:
        """GoogLeNet inception branches end relu -> concat: the ReLU's
        backward (dy *= x>0) folds into the concat's backward scatter
        (split_channels relu_masks), deleting one elementwise kernel per
        branch per step (36 of GoogLeNet's 65 relu_bwd launches). GPU,
        in-place slope-0 ReLUs, channel concat with vector-aligned widths
        and all-propagate bottoms only; PS_NO_CONCAT_MASK=1 disables (used
        by the equivalence test)."""
        import os
        if ctx().device != "cuda" or os.environ.get("PS_NO_CONCAT_MASK"):
            return
        p = self.param
        producer_layer: Dict[str, int] = {}
        for li, lp in enumerate(p.layers):
            for t in lp.top:
                producer_layer[t] = li
        vecw = 8 if ctx().compute_dtype == torch.bfloat16 else 4
        for ci, lp in enumerate(p.layers):
            if lp.enum_name("type") != "CONCAT":
                continue
            concat = self.layers[ci]
            if getattr(concat, "dim", 1) != 1:
                continue
            if not all(self.bottom_need_bwd[ci]):
                continue
            if any(b.channels % vecw for b in self.bottoms[ci]):
                continue  # masked path needs the aligned fused kernel
            mask_idx = set()
            for j, bname in enumerate(lp.bottom):
                pj = producer_layer.get(bname)
                if pj is None:
                    continue
                pl = p.layers[pj]
                relu = self.layers[pj]
                if (pl.enum_name("type") == "RELU"
                        and pl.top[0] == pl.bottom[0]  # in-place
                        and getattr(relu, "slope", 1.0) == 0.0
                        and relu.loss_weights[0] == 0.0):
                    mask_idx.add(j)
                    relu.bwd_fused_into_consumer = True
            if mask_idx:
                concat._mask_bottoms = mask_idx

    def _fuse_bwd_tails(self) -> None:
        """conv -> relu (in place) -> {lrn [-> max pool] | max pool | conv}:
        the backward of the layer after the ReLU writes the conv's top diff,
        so it also applies the ReLU mask and sums the conv's bias gradient
        in the same pass (ops.lrn_backward_tail / pool_max_backward_tail /
        relu_backward_bias). The ReLU's own backward, the pool's (under an
        LRN) and the conv's bias colsum disappear: AlexNet's conv1/conv2
        tails go from four memory-bound kernels over the conv output to one.
        GPU, slope-0 in-place ReLUs behind a single-top, single-bottom conv
        with a bias, vector-aligned channels, and a conv output of at least
        PS_BWD_TAIL_MIN_BYTES (default 16 MiB: below that the block
        reduction and atomics at the end of the fused kernel cost more than
        the share of the batched colsum_mt launch they replace -- GoogLeNet's
        21 small reduce convs lost 0.13 ms/step with it); everything else
        keeps the per-layer path. PS_NO_BWD_TAIL_FUSION=1 disables (tests,
        A/B runs); PS_MULTI_STREAM=1 also does (the bias gradient would be
        written from the consumer's stream)."""
        import os
        if (ctx().device != "cuda" or os.environ.get("PS_NO_BWD_TAIL_FUSION")
                or os.environ.get("PS_MULTI_STREAM", "0") == "1"):
            return
        p = self.param
        bf16 = ctx().compute_dtype == torch.bfloat16
        vecw = 8 if bf16 else 4
        min_count = int(os.environ.get("PS_BWD_TAIL_MIN_BYTES", 16 << 20)) \
            // (2 if bf16 else 4)

        def sole_consumer(name: str, after: int):
            """Index of the only layer reading blob `name` as produced by
            layer `after` (None if several, or none)."""
            found = None
            for lj in range(after + 1, len(p.layers)):
                if name in p.layers[lj].bottom:
                    if found is not None:
                        return None
                    found = lj
                if name in p.layers[lj].top and lj != found:
                    break  # a later producer re-binds the name
            return found

        for li, lp in enumerate(p.layers):
            relu = self.layers[li]
            if (lp.enum_name("type") != "RELU" or len(lp.bottom) != 1
                    or lp.top[0] != lp.bottom[0]
                    or getattr(relu, "slope", 1.0) != 0.0
                    or relu.loss_weights[0] != 0.0
                    or getattr(relu, "bwd_fused_into_consumer", False)
                    or not self.layer_need_bwd[li]
                    or not self.bottom_need_bwd[li][0]):
                continue
            name = lp.bottom[0]
            ci = next((lj for lj in range(li - 1, -1, -1)
                       if name in p.layers[lj].top), None)
            if ci is None or p.layers[ci].enum_name("type") != "CONVOLUTION":
                continue
            conv, clp = self.layers[ci], p.layers[ci]
            if (len(clp.top) != 1 or len(clp.bottom) != 1
                    or not conv.bias_term or conv.loss_weights[0] != 0.0
                    or not self.layer_need_bwd[ci]
                    or self.tops[ci][0].channels % vecw
                    or self.tops[ci][0].count < min_count
                    or any(ci < lj < li and name in p.layers[lj].bottom
                           for lj in range(ci + 1, li))):
                continue
            ki = sole_consumer(name, li)
            if ki is None or not self.layer_need_bwd[ki]:
                continue
            klp, cons = p.layers[ki], self.layers[ki]
            if len(klp.bottom) != 1 or not self.bottom_need_bwd[ki][0]:
                continue
            ktype = klp.enum_name("type")
            C = self.tops[ci][0].channels
            if (ktype == "LRN" and cons.region == "ACROSS_CHANNELS"
                    and cons.loss_weights[0] == 0.0
                    and klp.top[0] != klp.bottom[0]
                    and ops.lrn_v8_ok(C, cons.size)):
                cons._tail_conv = conv
                pi = sole_consumer(klp.top[0], ki)
                if pi is not None:
                    plp, pool = p.layers[pi], self.layers[pi]
                    if (plp.enum_name("type") == "POOLING"
                            and pool.method == "MAX" and len(plp.top) == 1
                            and pool.loss_weights[0] == 0.0
                            and self.layer_need_bwd[pi]
                            and self.bottom_need_bwd[pi][0]):
                        cons._tail_pool = pool
                        cons._tail_pool_top = self.tops[pi][0]
                        pool.bwd_fused_into_producer = True
                relu.bwd_fused_into_consumer = True
            elif (ktype == "POOLING" and cons.method == "MAX"
                  and len(klp.top) == 1 and cons.loss_weights[0] == 0.0):
                cons._tail_conv = conv
                relu.bwd_fused_into_consumer = True
            elif ktype == "CONVOLUTION":
                relu._tail_conv = conv  # the ReLU's own backward sums db
            else:
                continue
            conv.bias_grad_by_consumer = True

    def _build_stream_schedule(self, n_streams: int = 4) -> None:
        """Dataflow schedule for inter-branch stream parallelism.

        GoogLeNet's inception branches are independent chains whose GEMMs
        individually fill <20% of the 256 CUs; running sibling branches on
        separate HIP streams overlaps them. Assignment: a layer inherits
        its most recent producer's stream, except when that producer fans
        out to several consumers (a SPLIT) -- then siblings spread across
        the pool round-robin. Joins (CONCAT) wait on the other branches'
        events. insert_splits guarantees single-writer blob instances, so
        cross-stream hazards reduce to the recorded events plus
        record_stream() for the torch caching allocator."""
        L = len(self.layers)
        prods: List[List[int]] = [[] for _ in range(L)]
        last_writer: Dict[int, int] = {}
        for i in range(L):
            for b in self.bottoms[i]:
                j = last_writer.get(id(b))
                if j is not None and j not in prods[i]:
                    prods[i].append(j)
            for t in self.tops[i]:
                last_writer[id(t)] = i
        cons: List[List[int]] = [[] for _ in range(L)]
        for i in range(L):
            for pj in prods[i]:
                cons[pj].append(i)
        ls = [0] * L
        for i in range(L):
            if prods[i]:
                p0 = max(prods[i])
                sibs = cons[p0]
                ls[i] = sibs.index(i) % n_streams if len(sibs) > 1 else ls[p0]
        self._producers, self._consumers, self._lstream = prods, cons, ls
        # layers sharing a param blob must not race on its diff
        groups: Dict[int, List[int]] = {}
        for psp in self.params:
            groups.setdefault(psp.owner, []).append(psp.layer_idx)
        hazard = any(len({ls[li] for li in g}) > 1
                     for g in groups.values() if len(g) > 1)
        distinct = len(set(ls))
        self._ms_nstreams = n_streams if (distinct > 1 and not hazard) else 0

    def _ms_active(self) -> bool:
        """Opt-in (PS_MULTI_STREAM=1): branch overlap measured, but eager-
        mode host-side stream/event churn outweighs the GPU overlap on
        GoogLeNet (3.36k vs 4.00k img/s serial), and hipGraph capture of
        cross-stream event graphs segfaults inside ROCm 7.2 -- hipGraph
        (which already removes the launch gaps these streams target) is
        the winning configuration today."""
        import os
        if self._dbg_on:
            return False  # debug passes run the serial schedule
        return (self._ms_nstreams > 1 and ctx().device == "cuda"
                and torch.cuda.is_available()
                and os.environ.get("PS_MULTI_STREAM", "0") == "1")

    def _ms_streams(self):
        if self._ms_pool is None:
            self._ms_pool = [torch.cuda.Stream()
                             for _ in range(self._ms_nstreams - 1)]
            self._fwd_ev = [torch.cuda.Event() for _ in self.layers]
            self._bwd_ev = [torch.cuda.Event() for _ in self.layers]
        return [torch.cuda.current_stream()] + self._ms_pool

    def _fuse_relu_epilogues(self) -> None:
        """Fold an in-place slope-0 ReLU into the producing conv/IP GEMM
        epilogue. insert_splits guarantees each produced blob instance has
        a single consumer, so `top of conv == bottom of relu (in-place)`
        means the clamp commutes with nothing else. The ReLU layer stays
        in the net (its backward masks by the clamped activations, which
        is unchanged); its forward becomes a no-op. Mirrors cuDNN-style
        activation fusion; reference applied ReLU as a separate kernel
        (relu_layer.cu)."""
        p = self.param
        producer_of: Dict[str, int] = {}
        consumers: Dict[str, List[int]] = {}
        for li, lp in enumerate(p.layers):
            for t in lp.top:
                producer_of[t] = li  # in-place chains: latest producer wins
            for b in lp.bottom:
                consumers.setdefault(b, []).append(li)
        for li, lp in enumerate(p.layers):
            if lp.enum_name("type") != "RELU" or len(lp.bottom) != 1:
                continue
            if lp.top[0] != lp.bottom[0]:
                continue  # only in-place ReLU keeps backward semantics
            relu = self.layers[li]
            if relu.slope != 0.0 or relu.loss_weights[0] != 0.0:
                continue
            name = lp.bottom[0]
            # direct producer must be this blob's conv/IP (not another
            # in-place layer stacked in between)
            prod_li = None
            for lj in range(li - 1, -1, -1):
                if name in p.layers[lj].top:
                    prod_li = lj
                    break
            if prod_li is None:
                continue
            prod_lp = p.layers[prod_li]
            if prod_lp.enum_name("type") not in ("CONVOLUTION", "INNER_PRODUCT"):
                continue
            if len(prod_lp.top) != 1 or self.layers[prod_li].loss_weights[0] != 0.0:
                continue
            # the pre-ReLU value must not feed anything else: consumers
            # after the in-place ReLU read the post-ReLU instance (fine),
            # one strictly between producer and ReLU reads pre-ReLU (bad)
            if any(prod_li < lj < li for lj in consumers.get(name, [])):
                continue
            self.layers[prod_li].fuse_relu = True
            relu.fused = True

    # ------------------------------------------------------------------
    @property
    def learnable_params(self) -> List[ParamSpec]:
        return [ps for i, ps in enumerate(self.params) if ps.owner == i
                and ps.lr_mult != 0.0]

    def zero_param_diffs(self) -> None:
        owned = [ps.blob for i, ps in enumerate(self.params) if ps.owner == i]
        if owned and owned[0].data.is_cuda:
            # one zero_mt kernel instead of one zero_() launch per param
            # (GoogLeNet: 116 launches -> 1); diff tensors are identity-
            # stable after the first backward, so build the table once.
            # Layer-owned scratch that must start each iteration zeroed
            # (conv dwk buffers -- lets the split-K wgrad skip its memset)
            # rides in the same launch.
            extra = [t for l in self.layers
                     if hasattr(l, "extra_zero_buffers")
                     for t in l.extra_zero_buffers()]
            # A weight diff that its one writer overwrites in this backward
            # (the solver marks those layers) is not zeroed: 0 + dW is dW.
            # The identity key below follows the set.
            skip = {id(l.blobs[0]) for l in self.layers
                    if l.blobs and hasattr(l, "overwrites_dw")
                    and l.overwrites_dw()}
            zeroed = [b for b in owned if id(b) not in skip]
            if self._zero_mt is None and all(
                    b.has_diff() and b.diff.dtype == torch.float32
                    and b.diff.is_contiguous() for b in owned):
                ts = [b.diff for b in zeroed] + extra
                if not ts:
                    return
                self._zero_mt = (ops.zero_mt_prepare(ts), [id(t) for t in ts])
            if self._zero_mt is not None:
                mt, ids = self._zero_mt
                cur = [id(b.diff) for b in zeroed] + [id(t) for t in extra]
                if cur == ids:
                    ops.zero_mt_run(mt)
                    return
                self._zero_mt = None  # identity changed; rebuild next time
            for t in extra:
                t.zero_()
        for b in owned:
            b.zero_diff()

    def _flush_deferred_unpacks(self) -> None:
        """ONE unpack_mt kernel accumulates every conv's khwc wgrad scratch
        into its NCHW param diff (GoogLeNet: 57 weight_from_khwc launches
        -> 1). Active only when conv layers ran with defer_unpack (set by
        the solver in single-GPU mode -- DWBP needs per-layer grads final
        before the bucketed all-reduce fires)."""
        convs = [l for l in self.layers
                 if getattr(l, "_unpack_pending", False)]
        if not convs:
            return
        # a conv the solver marked writes its (un-zeroed) diff; the others
        # add to theirs
        over = [l.overwrites_dw() for l in convs]
        key = [(id(l._dwk_cache), id(l.blobs[0].diff), l._dwk_layout, o)
               for l, o in zip(convs, over)]
        if self._unpack_mt is None or self._unpack_mt[1] != key:
            self._unpack_mt = (ops.unpack_mt_prepare(
                [l._dwk_cache for l in convs],
                [l.blobs[0].diff for l in convs],
                [l.blobs[0].data.shape[1] for l in convs],
                [l.blobs[0].data.shape[2] for l in convs],
                [l.blobs[0].data.shape[3] for l in convs],
                [l._dwk_layout[0] for l in convs],
                [l._dwk_layout[1] for l in convs], over), key)
        ops.unpack_mt_run(self._unpack_mt[0])
        for l in convs:
            l._unpack_pending = False
        # deferred conv bias grads: one colsum_mt launch when the dy
        # identities held steady for a full iteration (the persistent
        # dgrad/split caches make them steady from iteration 2; eager
        # per-layer colsums cover the settling iterations so capture
        # never records a table upload)
        pend = [(l, l._pending_colsum) for l in self.layers
                if getattr(l, "_pending_colsum", None) is not None]
        if pend:
            # every entry already proved identity-stable (the layer only
            # defers after its dy pointer repeated), so build on first
            # sight of a new key -- the set settles by warmup iteration 3
            key = [(dy.data_ptr(), db.data_ptr(), tuple(dy.shape))
                   for _, (dy, db) in pend]
            # deterministic mode sizes the table's scratch at prepare time
            key.append(ops.conv_policy_epoch())
            if self._colsum_mt is None or self._colsum_mt[1] != key:
                self._colsum_mt = (ops.colsum_mt_prepare(
                    [dy for _, (dy, db) in pend],
                    [db for _, (dy, db) in pend]), key)
            ops.colsum_mt_run(self._colsum_mt[0],
                              pend[0][1][0].dtype == torch.bfloat16)
            for l, _ in pend:
                l._pending_colsum = None

    # -- fc shadows kept current by the solver's update kernel -----------
    def mark_fc_shadows_current(self, layers) -> None:
        """The solver's update just wrote these INNER_PRODUCT layers' bf16
        shadows from the new weights. Until a master changes again the
        repack skips them (the table without them is built here, outside
        any capture). The guard is torch's per-tensor _version: the update
        kernel writes through raw pointers and leaves it alone, while
        copy_ / load_weights / restore bump it."""
        if self._repack_mt is None or not layers:
            self._fc_marks = None
            return
        marks = [(l, l.blobs[0].data, l.blobs[0].data._version, l._wk_cache)
                 for l in layers]
        key = tuple(id(l) for l in layers)
        if self._repack_lite is None or self._repack_lite[1] != key:
            rest = [e for e in self._repack_entries
                    if all(e[0] is not l for l in layers)]
            mt = ops.repack_mt_prepare(*[[e[k] for e in rest]
                                         for k in range(1, 7)]) \
                if rest else None
            self._repack_lite = (mt, key)
        self._fc_marks = marks

    def invalidate_fc_shadows(self) -> None:
        self._fc_marks = None

    def fc_shadows_current(self) -> bool:
        """Whether every shadow the solver marked still matches its master:
        same tensors, same versions."""
        marks = self._fc_marks
        return (marks is not None and ops.fused_weight_tail()
                and all(l.blobs[0].data is m and m._version == v
                        and l._wk_cache is sh for l, m, v, sh in marks))

    def _maybe_mt_repack(self, full: bool = False) -> None:
        """One repack_mt kernel refreshes every conv's bf16 khwc shadow +
        dgrad transpose from the fp32 masters (GoogLeNet: 2 launches
        instead of 68 per step). Buffers are persistent per layer; the
        table is keyed on master identities (restore() rebuilds). While the
        fc shadows the solver marked are current (and full is False) the
        table without them runs instead."""
        if ctx().device != "cuda" or ctx().compute_dtype != torch.bfloat16:
            return
        convs = [l for l in self.layers
                 if l.type_name == "CONVOLUTION" and l.blobs
                 and l.blobs[0].data.is_cuda
                 and l.blobs[0].data.dtype == torch.float32]
        ips = [l for l in self.layers
               if l.type_name == "INNER_PRODUCT" and l.blobs
               and l.blobs[0].data.is_cuda
               and l.blobs[0].data.dtype == torch.float32]
        if not convs and not ips:
            return
        # the policy epoch: a conv-policy setter may have changed a plan's
        # khwc layout since the shadows were sized
        key = [id(l.blobs[0].data) for l in convs + ips]
        key.append(ops.conv_policy_epoch())
        if self._repack_mt is None or self._repack_key != key:
            masters, wks, wkTs, Gs, kw_lds, c_lds = [], [], [], [], [], []
            for l in convs:
                w = l.blobs[0].data
                Co, Cig, kh, kw = w.shape
                G = l.group
                # the width and khwc layout conv2d_forward_ex plans for (it
                # rejects another width). Columns the repack never writes
                # (pad columns, a packed first layer's unused channel slots
                # and phantom taps) are zeroed here, once.
                x_shape = self.bottoms[self.layers.index(l)][0].shape
                plan = ops.conv_plan(x_shape, w.shape, l.stride, l.pad, G,
                                     bf16=True)
                wk_ld = plan["wk_ld"]
                kw_lds.append(plan["kw_ld"])
                c_lds.append(plan["c_ld"])
                wk = torch.zeros(Co, wk_ld, dtype=torch.bfloat16,
                                 device=w.device)
                wkT = torch.empty(G * kh * kw * Cig, Co // G,
                                  dtype=torch.bfloat16, device=w.device)
                l._wk_cache = (wk, wkT)
                masters.append(w)
                wks.append(wk)
                wkTs.append(wkT)
                Gs.append(G)
            for l in ips:
                # IP shadows ride the same table: masters viewed (N,K,1,1)
                # make the khwc layout degenerate to row-major [N][K]; the
                # transpose output is skipped (empty wkT)
                w = l.blobs[0].data  # (1,1,N,K) contiguous
                wk = torch.empty(l.N, l.K, dtype=torch.bfloat16,
                                 device=w.device)
                l._wk_cache = wk
                masters.append(w.view(l.N, l.K, 1, 1))
                wks.append(wk)
                wkTs.append(torch.empty(0, dtype=torch.bfloat16,
                                        device=w.device))
                Gs.append(1)
                kw_lds.append(1)
                c_lds.append(l.K)
            self._repack_mt = ops.repack_mt_prepare(masters, wks, wkTs, Gs,
                                                    kw_lds, c_lds)
            self._repack_key = key
            # new shadow buffers: nothing the solver wrote is in them
            self._repack_entries = list(zip(convs + ips, masters, wks, wkTs,
                                            Gs, kw_lds, c_lds))
            self._repack_lite = None
            self._fc_marks = None
        if not full and self.fc_shadows_current():
            if self._repack_lite[0] is not None:
                ops.repack_mt_run(self._repack_lite[0])
            return
        self._fc_marks = None
        ops.repack_mt_run(self._repack_mt)

    # -- debug_info ------------------------------------------------------
    def set_debug_info(self, on: bool) -> None:
        """Per-layer blob statistics for the passes that follow (reference
        Net::set_debug_info). Read them back with debug_records()."""
        self._dbg_on = bool(on)
        if self._dbg_on and self._dbg is None:
            from .debug_info import DebugInfo
            self._dbg = DebugInfo(self)

    @property
    def debug_info(self) -> bool:
        return self._dbg_on

    def debug_records(self) -> List[dict]:
        """Records of the last pass run with debug_info on: one device-to-
        host copy of the statistics buffer."""
        return self._dbg.records() if self._dbg is not None else []

    def debug_param_diffs(self) -> None:
        """Take the param-diff statistics now (the distributed solver, after
        its all-reduce; a local backward() does it itself)."""
        if self._dbg_on:
            self._dbg.param_diffs()

    def forward(self, start: int = 0, end: Optional[int] = None) -> float:
        end = len(self.layers) if end is None else end
        self._maybe_mt_repack()
        dbg = self._dbg if self._dbg_on else None
        if dbg is not None:
            dbg.begin()
        loss = 0.0
        for i in range(start, end):
            self.layers[i].forward(self.bottoms[i], self.tops[i])
            if dbg is not None:
                dbg.tops(i)
            for (li, ti, w) in self._loss_tops:
                if li == i:
                    loss += w * float(self.tops[i][ti].data.sum().item())
        if dbg is not None:
            dbg.end_forward()
        return loss

    def forward_async(self) -> torch.Tensor:
        """Forward pass without host synchronization: returns the loss as a
        0-d device tensor (sum of weighted loss tops)."""
        dev = ctx().torch_device
        self._maybe_mt_repack()
        if self._ms_active():
            self._forward_ms()
            loss = torch.zeros((), dtype=torch.float32, device=dev)
            for (li, ti, w) in self._loss_tops:
                loss = loss + w * self.tops[li][ti].data.sum().to(torch.float32)
            return loss
        loss = torch.zeros((), dtype=torch.float32, device=dev)
        marks = self._loss_marks
        layers = self.layers
        bottoms = self.bottoms
        tops = self.tops
        dbg = self._dbg if self._dbg_on else None
        if dbg is not None:
            dbg.begin()
        for i in range(len(layers)):
            layers[i].forward(bottoms[i], tops[i])
            if dbg is not None:
                dbg.tops(i)
            if i in marks:
                for (ti, w) in marks[i]:
                    loss = loss + w * tops[i][ti].data.sum().to(torch.float32)
        if dbg is not None:
            dbg.end_forward()
        return loss

    def _forward_ms(self) -> None:
        """Forward with sibling branches on separate HIP streams. The main
        (current) stream is stream 0; every cross-stream read waits the
        producer's event and record_stream()s the tensor for the caching
        allocator; the main stream joins every used stream at the end."""
        streams = self._ms_streams()
        ls = self._lstream
        # record_stream is allocator bookkeeping for cross-stream tensor
        # lifetime; under hipGraph capture the graph pool freezes addresses,
        # and calling it there aborts the capture
        rec = not torch.cuda.is_current_stream_capturing()
        last_on_stream: Dict[int, int] = {}
        for i, layer in enumerate(self.layers):
            s = streams[ls[i]]
            for pj in self._producers[i]:
                if ls[pj] != ls[i]:
                    s.wait_event(self._fwd_ev[pj])
            with torch.cuda.stream(s):
                if rec:
                    for b in self.bottoms[i]:
                        b.data.record_stream(s)
                layer.forward(self.bottoms[i], self.tops[i])
            self._fwd_ev[i].record(s)
            last_on_stream[ls[i]] = i
        cur = streams[0]
        for k, li in last_on_stream.items():
            if k != 0:
                cur.wait_event(self._fwd_ev[li])

    def backward(self, post_layer_cb: Optional[Callable[[int, Layer], None]] = None
                 ) -> None:
        """Run backward over all layers that need it.

        post_layer_cb(layer_idx, layer) fires right after a layer's backward
        -- the DWBP hook: by this point the layer's param diffs are final and
        gradient comm may be enqueued while backprop continues below.
        """
        # seed loss-top diffs with their loss weights
        for (li, ti, w) in self._loss_tops:
            t = self.tops[li][ti]
            t.diff.fill_(w)
        if self._ms_active():
            self._backward_ms(post_layer_cb)
            self._flush_deferred_unpacks()
            return
        dbg = self._dbg if self._dbg_on else None
        for i in range(len(self.layers) - 1, -1, -1):
            if not self.layer_need_bwd[i]:
                continue
            self.layers[i].backward(self.tops[i], self.bottom_need_bwd[i],
                                    self.bottoms[i])
            if dbg is not None:
                dbg.bottoms(i)
            if post_layer_cb is not None and self.layers[i].blobs:
                post_layer_cb(i, self.layers[i])
        self._flush_deferred_unpacks()
        # param diffs are final only here (deferred unpacks, batched colsum)
        if dbg is not None and not self._dbg_defer_param_diffs:
            dbg.param_diffs()

    def _backward_ms(self, post_layer_cb) -> None:
        """Backward mirror of _forward_ms: layer i runs on its forward
        stream, waiting the backward events of every consumer on another
        stream (their backward wrote this layer's top diffs)."""
        streams = self._ms_streams()
        ls = self._lstream
        # loss-top diff seeding above ran on the main stream; branch streams
        # with a loss layer (aux heads) have no consumer event to wait on,
        # so fork them explicitly from the seed point
        seed_ev = torch.cuda.Event()
        seed_ev.record(streams[0])
        for st in streams[1:]:
            st.wait_event(seed_ev)
        rec = not torch.cuda.is_current_stream_capturing()
        ran = [False] * len(self.layers)
        last_on_stream: Dict[int, int] = {}
        for i in range(len(self.layers) - 1, -1, -1):
            if not self.layer_need_bwd[i]:
                continue
            s = streams[ls[i]]
            for cj in self._consumers[i]:
                if ran[cj] and ls[cj] != ls[i]:
                    s.wait_event(self._bwd_ev[cj])
            with torch.cuda.stream(s):
                if rec:
                    for t in self.tops[i]:
                        if t.has_diff():
                            t.diff.record_stream(s)
                self.layers[i].backward(self.tops[i],
                                        self.bottom_need_bwd[i],
                                        self.bottoms[i])
                if post_layer_cb is not None and self.layers[i].blobs:
                    post_layer_cb(i, self.layers[i])
            self._bwd_ev[i].record(s)
            ran[i] = True
            last_on_stream[ls[i]] = i
        cur = streams[0]
        for k, li in last_on_stream.items():
            if k != 0:
                cur.wait_event(self._bwd_ev[li])

    def clear_activation_diffs(self) -> None:
        """Zero intermediate blob diffs between iterations (layers accumulate
        into bottom diffs where blobs fan out via splits)."""
        for b in self.blobs.values():
            if b.has_diff():
                b.zero_diff()

    # -- checkpoint interop --------------------------------------------
    def to_proto(self, write_diff: bool = False) -> Message:
        out = Message.decode("NetParameter", self.param.encode())
        for li, lp in enumerate(out.layers):
            del lp.blobs[:]
            for pblob in self.layers[li].blobs:
                lp.blobs.append(pblob.to_proto(write_diff))
        return out

    def copy_trained_layers_from(self, src: Message) -> None:
        """Load weights by layer name (net.cpp:908-950)."""
        by_name = {l.name: l for l in self.layers}
        for lp in src.layers:
            layer = by_name.get(lp.name)
            if layer is None:
                continue
            src_blobs = list(lp.blobs)
            if not src_blobs:
                continue
            if len(src_blobs) != len(layer.blobs):
                raise ValueError(
                    f"layer {lp.name}: {len(src_blobs)} checkpoint blobs vs "
                    f"{len(layer.blobs)} params")
            for pb, sb in zip(layer.blobs, src_blobs):
                pb.from_proto(sb, reshape=False)

    def blob(self, name: str) -> Blob:
        return self.blobs[name]

    def has_layer_type(self, type_name: str) -> bool:
        return any(l.type_name == type_name for l in self.layers)

"""Per-GPU Node runtime: one process per MI355X, one pipeline stage per
process, RCCL channels between stages.

Capability parity with the reference's Node (ravnest/node.py:23-783):
role dispatch (root/stem/leaf), bounded in-flight async pipeline, action
handlers (root_forward/forward/backward/find_loss/no_grad variants/
save_submodel), periodic DP parameter averaging, latest-weights pull,
submodel save cascade. Differences are deliberate MI355X-first design:

* transport is RCCL P2P over xGMI (comm/p2p.py), not gRPC + pickle; the
  gRPC server subprocess + mp.Manager buffers (node.py:259-328,
  endpoints.py) are replaced by listener threads + an event-driven
  dispatch queue (no busy-poll);
* producers send outputs DIRECTLY to each consumer stage (skip
  connections included), so the reference's hop-by-hop payload forwarding
  and pass-through grad accumulation (node.py:533-540) become direct
  grad messages that the producer sums per output;
* DP parameter averaging is a bucketed RCCL all_reduce on the per-stage
  communicator (comm/collectives.py), not a hand-rolled chunked ring.
"""
from __future__ import annotations

import itertools
import json
import queue
import threading
import time
from pathlib import Path

import torch

from ..comm import CommBackend, Message
from ..comm.collectives import (AsyncReducer,
                                average_parameters,
                                average_optimizer_state,
                                average_parameter_segments,
                                _master_tensors)
from ..strings import ActionTypes, NodeTypes
from ..utils import load_node_json_configs
from .compute import ComputeEngine

_MAX_OUTS = 1024
_MODEL_INPUT_BASE = 1 << 20

# output_type codes carried in Message.extra for NO_GRAD_FORWARD
_OUT_TYPES = {"val_accuracy": 0, "accuracy": 1, "prediction": 2}
_OUT_TYPES_REV = {v: k for k, v in _OUT_TYPES.items()}


def _dtype_from_str(s: str) -> torch.dtype:
    return getattr(torch, s.replace("torch.", ""))


class _CyclingIterator:
    """Auto-resetting DataLoader iterator (the leaf's label feed must
    survive epoch boundaries; parity: reference labels iterator,
    node.py:144-163).

    LAZY: iter() is deferred to the first __next__. A seeded shuffling
    DataLoader draws its epoch permutation from its torch.Generator at
    iter() time; an eager draw at Node init desynchronized the root's
    training order from the leaf's labels whenever both wrap the same
    loader object (the walkthrough pattern) — the root's Trainer then
    iterated the generator's SECOND permutation against the leaf's
    FIRST, and the model could only learn the output mean."""

    def __init__(self, loader):
        self.loader = loader
        self.it = None
        self.wrapped = False  # set when the iterator wrapped (epoch end)

    def take_wrapped(self) -> bool:
        w, self.wrapped = self.wrapped, False
        return w

    def __next__(self):
        if self.loader is None:
            return None
        if self.it is None:
            self.it = iter(self.loader)
        try:
            return next(self.it)
        except StopIteration:
            self.it = iter(self.loader)
            self.wrapped = True
            return next(self.it)


class Node:
    def __init__(self, name: str | None = None,
                 base_dir: str = "node_data",
                 config: dict | None = None,
                 model: torch.nn.Module | None = None,
                 input_template: list | None = None,
                 output_template: dict | None = None,
                 optimizer=None,
                 optimizer_params: dict | None = None,
                 lr_scheduler=None,
                 lr_scheduler_params: dict | None = None,
                 lr_step_on_epoch_change: bool = True,
                 device: torch.device | None = None,
                 criterion=None,
                 labels=None,
                 test_labels=None,
                 update_frequency: int = 1,
                 reduce_factor: int | None = None,
                 average_optim: bool = False,
                 loss_filename: str = "losses.txt",
                 backend: str | None = None,
                 master_addr: str = "127.0.0.1",
                 master_port: int = 29500,
                 comm: CommBackend | None = None,
                 compression: bool = False,
                 wire_dtype: torch.dtype | None = None,
                 amp_dtype: torch.dtype | None = None,
                 async_reduce: bool = True,
                 model_transform=None,
                 max_grad_norm: float | None = None):
        # parity: the reference's fp16 wire compression (utils.py:184-194)
        # becomes an optional on-the-wire cast; bf16 is the natural MI355X
        # wire dtype (no clamping needed)
        if compression and wire_dtype is None:
            wire_dtype = torch.bfloat16
        self.wire_dtype = wire_dtype
        self.base_dir = base_dir
        if config is None:
            config = load_node_json_configs(name, base_dir)
        self.config = config
        self.rank = config["rank"]
        self.world_size = config["world_size"]
        self.cluster_id = config.get("cluster_id", 0)
        self.stage = config.get("stage", 0)
        self.n_stages = config.get("n_stages", 1)
        self.cluster_length = config.get("cluster_length", self.n_stages)
        self.stage_ranks = config.get("stage_ranks", [self.rank])
        self.dp_ranks = config.get("dp_ranks", [self.rank])
        self.node_type = NodeTypes(config.get("node_type", "root"))
        self.template_path = config.get("template_path")
        self.name = config.get("name", f"node_{self.rank}")

        if device is not None:
            self.device = torch.device(device)
        elif torch.cuda.is_available():
            local = int(__import__("os").environ.get(
                "LOCAL_RANK", self.rank % max(1, torch.cuda.device_count())))
            self.device = torch.device("cuda", local)
        else:
            self.device = torch.device("cpu")

        self.fused = self.n_stages == 1  # root==leaf: whole model on 1 GPU

        # ---- model & templates --------------------------------------
        if model is None:
            model = torch.load(Path(self.template_path) / "submod.pt",
                               map_location="cpu", weights_only=False)
        if model_transform is not None:
            # applied BEFORE optimizer/engine init (e.g. .to(bfloat16)
            # for bf16-native pipeline stages — bench.py --parallelism pp)
            model = model_transform(model)
        self.model = model.to(self.device)
        if input_template is None and self.template_path:
            with open(Path(self.template_path) / "inputs.json") as f:
                input_template = json.load(f)
        if output_template is None and self.template_path:
            with open(Path(self.template_path) / "outputs.json") as f:
                output_template = {int(k): v for k, v in json.load(f).items()}
        self.input_template = input_template or []
        self.output_template = output_template or {}
        if config.get("model_input_names"):
            self.model_input_names = config["model_input_names"]
        else:
            mi_path = Path(base_dir) / "model_inputs.json"
            if mi_path.exists():
                with open(mi_path) as f:
                    self.model_input_names = json.load(f)["input_names"]
            else:
                self.model_input_names = []

        # ---- optimizer / engine -------------------------------------
        optimizer_params = optimizer_params or {}
        opt = None
        if optimizer is not None:
            opt = optimizer(self.model.parameters(), **optimizer_params)
        self.optimizer = opt
        # per-node lr scheduler: built HERE so stem/leaf ranks step it too
        # (parity: reference node.py:213-215,517-518,585-586,603-604 —
        # a Trainer-owned scheduler would only ever run on the root)
        self.lr_scheduler = None
        self.lr_step_on_epoch_change = lr_step_on_epoch_change
        if lr_scheduler is not None and opt is not None:
            self.lr_scheduler = lr_scheduler(opt,
                                             **(lr_scheduler_params or {}))
        self.criterion = criterion
        self.labels = _CyclingIterator(labels)
        self.test_labels = _CyclingIterator(test_labels)
        self.update_frequency = update_frequency
        self.reduce_factor = reduce_factor
        self.reduce_threshold = (update_frequency * reduce_factor
                                 if reduce_factor else None)
        self.average_optim = average_optim
        self.loss_filename = loss_filename
        self.engine = ComputeEngine(self.model, opt, self.device,
                                    update_frequency=update_frequency,
                                    criterion=criterion,
                                    loss_filename=loss_filename,
                                    amp_dtype=amp_dtype,
                                    versioning=not self.fused,
                                    max_grad_norm=max_grad_norm)

        # ---- routing precomputation ---------------------------------
        self._build_routing()

        # ---- pipeline state -----------------------------------------
        self.forward_pass_id = 0
        self.eval_pass_id = 0
        self.latest_backward_id = -1
        self._backward_done = threading.Condition()
        self._pending_fwd: dict[tuple, dict] = {}
        self._pending_grads: dict[int, dict] = {}
        self._pending_lock = threading.Lock()
        self._actions: queue.PriorityQueue = queue.PriorityQueue()
        self._action_seq = itertools.count()
        self._stop = threading.Event()
        self._weights_reply_q: queue.Queue = queue.Queue()
        self.losses: list[float] = []
        self.val_accuracies: list[float] = []

        # ---- comm ----------------------------------------------------
        if comm is not None:
            self.comm = comm
        elif self.world_size > 1:
            self.comm = CommBackend(
                rank=self.rank, world_size=self.world_size,
                base_dir=base_dir, device=self.device, backend=backend,
                master_addr=master_addr, master_port=master_port)
        else:
            self.comm = None
        self.comm_session = _CommSessionFacade(self)

        # overlapped DP averaging: collective launched on a side stream
        # at the reduce threshold, joined (via engine.pre_step_hook)
        # right before the next optimizer step — the reduce rides under
        # the next microbatch's compute instead of blocking the pipeline
        # (SURVEY.md §7 "Overlap engineering"; the reference blocks).
        self._reducer = None
        if (async_reduce
                and __import__("os").environ.get(
                    "RAVNEST_ASYNC_REDUCE", "1") == "1"
                and self.comm is not None
                and len(self.dp_ranks) > 1
                and not getattr(self.comm, "my_dp_segments", None)):
            self._reducer = AsyncReducer(self.comm.my_dp_group, self.device)
            self.engine.pre_step_hook = self._join_reduce

        self._mem_log = __import__("os").environ.get(
            "RAVNEST_MEM_LOG", "0") == "1"
        self._dispatch_thread: threading.Thread | None = None
        self._started = False
        self.health_monitor = None

    def _join_reduce(self):
        if self._reducer is not None and self._reducer.pending:
            self._reducer.join_into()
            self.engine.bump_version()

    def join_pending_reduce(self):
        """Drain any in-flight overlapped DP reduce (checkpoints, weight
        serving, shutdown)."""
        self._join_reduce()

    # ==================================================================
    # aux subsystems (health, checkpoint) — SURVEY.md section 5 parity+
    # ==================================================================
    def start_health_monitor(self, interval: float = 2.0,
                             timeout: float = 10.0, on_peer_lost=None,
                             on_peer_recovered=None):
        """Heartbeat over the ctrl channels. Default recovery policy
        (parity+: the reference only ships an unused Ping RPC): when a
        DP replica goes silent, parameter averaging is DISABLED so
        training continues un-averaged instead of hanging the next
        collective on the dead rank; when the peer's heartbeat returns,
        averaging re-enables (the rejoining rank pulls weights via
        update_with_latest_weights — the elastic-join path)."""
        from .health import HealthMonitor
        self.health_monitor = HealthMonitor(
            self, interval=interval, timeout=timeout,
            on_peer_lost=on_peer_lost or self._on_dp_peer_lost,
            on_peer_recovered=on_peer_recovered or self._on_dp_peer_back)
        self.health_monitor.start()
        return self.health_monitor

    def _on_dp_peer_lost(self, peer: int):
        if peer in self.dp_ranks:
            self._dp_suspended = True
            print(f"[rank {self.rank}] DP peer {peer} lost — parameter "
                  "averaging suspended (training continues un-averaged)",
                  flush=True)

    def _on_dp_peer_back(self, peer: int):
        if peer in self.dp_ranks and getattr(self, "_dp_suspended", False):
            self._dp_suspended = False
            print(f"[rank {self.rank}] DP peer {peer} recovered — "
                  "parameter averaging resumed", flush=True)

    def health(self) -> dict:
        return (self.health_monitor.health()
                if self.health_monitor is not None else {"peers": {}})

    def save_checkpoint(self, path=None):
        self._join_reduce()
        from .checkpoint import save_checkpoint
        return save_checkpoint(self, path)

    def load_checkpoint(self, path=None):
        from .checkpoint import load_checkpoint
        return load_checkpoint(self, path)

    # ==================================================================
    # routing tables
    # ==================================================================
    def _build_routing(self):
        """Precompute, from the templates: per-input source rank/gid,
        per-output consumer ranks, expected grad contributions."""
        self.root_rank = self.stage_ranks[0]
        # one gid may feed several input positions (an output consumed
        # twice by this stage); the producer sends the tensor once
        self._gid_to_pos: dict[int, list[int]] = {}
        self._pos_src_rank: dict[int, int] = {}
        self._needs_grad: list[bool] = []
        self._pos_to_producer: dict[int, tuple[int, int, int]] = {}
        self._n_remote_inputs = 0
        self._local_positions: list[int] = []

        for pos, src in enumerate(self.input_template):
            kind = src.get("kind")
            if src.get("pyscalar"):
                floaty = False
            else:
                dtype_s = src.get("dtype", "torch.float32")
                floaty = _dtype_from_str(dtype_s).is_floating_point
            if kind == "stage":
                j = src["stage"]
                k = src.get("out_idx", 0)
                gid = j * _MAX_OUTS + k
                src_rank = self.stage_ranks[j]
                self._needs_grad.append(bool(floaty))
                self._pos_to_producer[pos] = (src_rank, j, k)
            elif kind == "model_input":
                idx = (self.model_input_names.index(src["name"])
                       if src["name"] in self.model_input_names else 0)
                gid = _MODEL_INPUT_BASE + idx
                src_rank = self.root_rank
                self._needs_grad.append(False)
            else:  # const
                self._needs_grad.append(False)
                self._local_positions.append(pos)
                continue
            first_use = gid not in self._gid_to_pos
            self._gid_to_pos.setdefault(gid, []).append(pos)
            self._pos_src_rank[pos] = src_rank
            if src_rank != self.rank:
                if first_use:
                    self._n_remote_inputs += 1  # tensor arrives once per gid
            else:
                self._local_positions.append(pos)

        # outputs: consumers grouped by rank; expected grad contributions
        self._out_consumers: dict[int, list[int]] = {}  # out_idx -> ranks
        self._expected_grad_contribs: dict[int, int] = {}
        for k, entry in self.output_template.items():
            ranks = []
            for cons in entry.get("consumers", []):
                j = cons["stage"]
                if j != self.stage:
                    ranks.append(self.stage_ranks[j])
            self._out_consumers[k] = ranks
            if entry.get("pyscalar"):
                floaty = False
            else:
                floaty = _dtype_from_str(
                    entry.get("dtype", "torch.float32")).is_floating_point
            self._expected_grad_contribs[k] = len(ranks) if floaty else 0
        self._total_expected_grads = sum(self._expected_grad_contribs.values())

        # model inputs this root must forward to later stages:
        # recomputed lazily from other stages' templates at plan time is
        # encoded in the comm edge list; the root resolves targets from
        # all stage input templates on disk.
        self._model_input_targets: dict[str, list[tuple[int, int]]] = {}
        if self.node_type == NodeTypes.ROOT and self.template_path:
            base = Path(self.base_dir)
            for s in range(1, self.n_stages):
                p = base / f"cluster_{self.cluster_id}" / f"stage_{s}" / "inputs.json"
                if not p.exists():
                    continue
                with open(p) as f:
                    tmpl = json.load(f)
                for src in tmpl:
                    if src.get("kind") == "model_input":
                        self._model_input_targets.setdefault(
                            src["name"], []).append(
                                (self.stage_ranks[s],
                                 _MODEL_INPUT_BASE +
                                 (self.model_input_names.index(src["name"])
                                  if src["name"] in self.model_input_names
                                  else 0)))

    # ==================================================================
    # lifecycle
    # ==================================================================
    def start(self):
        if self._started:
            return
        self._started = True
        if self.comm is not None:
            self.comm.start(self._deliver)
        self._dispatch_thread = threading.Thread(
            target=self._dispatch_loop, daemon=True,
            name=f"dispatch:rank{self.rank}")
        self._dispatch_thread.start()

    def stop(self):
        # drain any in-flight overlapped DP reduce first: tearing down
        # process groups under a live side-stream collective aborts
        try:
            self.join_pending_reduce()
        except Exception:
            pass
        self._stop.set()
        self._enqueue(2, ("_stop", None, None))
        if self.comm is not None:
            self.comm.stop()

    # ==================================================================
    # message delivery (listener threads) -> assembly -> action queue
    # ==================================================================
    def _enqueue(self, prio: int, item):
        self._actions.put((prio, next(self._action_seq), item))

    def _deliver(self, channel, msg: Message):
        if msg.action in (ActionTypes.FORWARD, ActionTypes.NO_GRAD_FORWARD):
            self._assemble_forward(msg)
        elif msg.action == ActionTypes.BACKWARD:
            self._assemble_backward(msg)
        elif msg.action == ActionTypes.SAVE_SUBMODEL:
            self._enqueue(1, ("save_submodel", None, None))
        elif msg.action == ActionTypes.STOP:
            if msg.extra == 3:  # health PING -> reply PONG on ctrl
                if self.health_monitor is not None:
                    self.health_monitor.note_ping(channel.src)
                try:
                    self.comm.send(channel.src, "ctrl", Message(
                        action=ActionTypes.STOP, fpid=-2, tensors=[],
                        extra=4))
                except KeyError:
                    pass
            elif msg.extra == 4:  # PONG
                if self.health_monitor is not None:
                    self.health_monitor.note_pong(channel.src)
            else:
                self._enqueue(3, ("stop_cascade", None, None))
        elif msg.action == ActionTypes.PREDICTION and channel.kind == "ctrl":
            # WEIGHTS protocol over ctrl: extra==1 request (optionally
            # carrying a newline-joined param-NAME blob for a partial
            # range), extra==2 reply
            if msg.extra == 1:
                self._enqueue(1, ("weights_request", channel.src,
                                  msg.tensors))
            else:
                self._weights_reply_q.put(msg.tensors)

    def _assemble_forward(self, msg: Message):
        is_eval = msg.action == ActionTypes.NO_GRAD_FORWARD
        key = (is_eval, msg.fpid)
        with self._pending_lock:
            ent = self._pending_fwd.setdefault(
                key, {"tensors": {}, "gids": set(), "extra": msg.extra})
            for gid, t in msg.tensors:
                for pos in self._gid_to_pos.get(gid, ()):
                    ent["tensors"][pos] = t
                ent["gids"].add(gid)
            if msg.extra:
                ent["extra"] = msg.extra
            done = len(ent["gids"]) >= self._n_remote_inputs
            if done:
                del self._pending_fwd[key]
        if done:
            action = (ActionTypes.NO_GRAD_FORWARD if is_eval
                      else ActionTypes.FORWARD)
            self._enqueue(1, (str(action), msg.fpid,
                              {"tensors": ent["tensors"],
                               "extra": ent["extra"]}))

    def _assemble_backward(self, msg: Message):
        with self._pending_lock:
            ent = self._pending_grads.setdefault(
                msg.fpid, {"grads": {}, "count": 0, "extra": 0})
            for gid, g in msg.tensors:
                k = gid % _MAX_OUTS
                if k in ent["grads"]:
                    ent["grads"][k] = ent["grads"][k] + g
                else:
                    ent["grads"][k] = g
                ent["count"] += 1
            ent["extra"] |= msg.extra
            done = ent["count"] >= self._total_expected_grads
            if done:
                del self._pending_grads[msg.fpid]
        if done:
            self._enqueue(0, (str(ActionTypes.BACKWARD), msg.fpid, ent))

    # ==================================================================
    # dispatch loop
    # ==================================================================
    def _dispatch_loop(self):
        while not self._stop.is_set():
            try:
                _, _, item = self._actions.get(timeout=1.0)
            except queue.Empty:
                continue
            kind, fpid, payload = item
            if kind == "_stop":
                return
            try:
                self._dispatch(kind, fpid, payload)
            except Exception:
                import traceback
                traceback.print_exc()
                self._stop.set()
                raise

    def _dispatch(self, kind: str, fpid, payload):
        if kind == str(ActionTypes.FORWARD):
            if self.node_type == NodeTypes.LEAF and not self.fused:
                self._handle_find_loss(fpid, payload)
            else:
                self._handle_forward(fpid, payload)
        elif kind == str(ActionTypes.BACKWARD):
            self._handle_backward(fpid, payload)
        elif kind == str(ActionTypes.NO_GRAD_FORWARD):
            self._handle_no_grad_forward(fpid, payload)
        elif kind == str(ActionTypes.ROOT_FORWARD):
            self._handle_root_forward(fpid, payload)
        elif kind == "root_no_grad":
            self._handle_root_no_grad(fpid, payload)
        elif kind == "save_submodel":
            self._handle_save()
        elif kind == "weights_request":
            self._handle_weights_request(payload_src=fpid,
                                         req_tensors=payload)
        elif kind == "stop_cascade":
            self._forward_stop()
            self._stop.set()

    # ==================================================================
    # argument assembly helpers
    # ==================================================================
    def _build_args(self, tensors_by_pos: dict[int, torch.Tensor],
                    model_inputs: dict | None = None) -> list:
        args = []
        for pos, src in enumerate(self.input_template):
            kind = src.get("kind")
            if kind == "const":
                args.append(src.get("value"))
            elif pos in tensors_by_pos:
                t = tensors_by_pos[pos]
                if src.get("pyscalar") and torch.is_tensor(t):
                    args.append(int(t.item()))
                elif torch.is_tensor(t):
                    t = t.to(self.device)
                    # decompress wire-cast activations to the template
                    # dtype (parity: reference compute.py:160-163) —
                    # ONLY when compression actually converted them. The
                    # templates record PLAN-time dtypes (fp32 trace); a
                    # bf16-native stage must receive its neighbor's bf16
                    # hidden states as-is, not upcast to the plan dtype
                    # (that fed fp32 into bf16 Linears on the first real
                    # GPU pipeline run).
                    want = src.get("dtype")
                    if (self.wire_dtype is not None and want
                            and t.is_floating_point()
                            and t.dtype == self.wire_dtype):
                        wd = _dtype_from_str(want)
                        if wd.is_floating_point and t.dtype != wd:
                            t = t.to(wd)
                    args.append(t)
                else:
                    args.append(t)
            elif kind == "model_input" and model_inputs is not None:
                args.append(model_inputs[src["name"]])
            else:
                raise RuntimeError(
                    f"rank {self.rank}: missing input pos {pos} ({src})")
        return args

    def _send_outputs(self, action: ActionTypes, fpid: int, outputs: tuple,
                      extra: int = 0):
        """Group outputs per consumer rank into one message each."""
        by_rank: dict[int, list] = {}
        for k, ranks in self._out_consumers.items():
            if k >= len(outputs):
                continue
            out = outputs[k]
            if torch.is_tensor(out):
                out = out.detach()
                if self.wire_dtype is not None and out.is_floating_point():
                    out = out.to(self.wire_dtype)
            else:  # routed python scalar (a .size() value): ship as int64
                out = torch.tensor([int(out)], dtype=torch.int64,
                                   device=self.device)
            for r in set(ranks):
                by_rank.setdefault(r, []).append(
                    (self.stage * _MAX_OUTS + k, out))
        for r, tensors in by_rank.items():
            self.comm.send(r, "fwd", Message(action=action, fpid=fpid,
                                             tensors=tensors, extra=extra))

    def _send_input_grads(self, fpid: int, input_grads: list,
                          extra: int = 0):
        by_rank: dict[int, list] = {}
        for pos, g in enumerate(input_grads):
            if g is None or pos not in self._pos_to_producer:
                continue
            src_rank, j, k = self._pos_to_producer[pos]
            if src_rank == self.rank:
                continue
            # grads ride the wire at wire_dtype too (parity: reference
            # compresses both directions, utils.py:184-194; the engine
            # casts back to the output dtype at the consumer,
            # compute.py backward g.to(out.dtype))
            if self.wire_dtype is not None and g.is_floating_point():
                g = g.to(self.wire_dtype)
            by_rank.setdefault(src_rank, []).append((j * _MAX_OUTS + k, g))
        for r, tensors in by_rank.items():
            self.comm.send(r, "bwd", Message(action=ActionTypes.BACKWARD,
                                             fpid=fpid, tensors=tensors,
                                             extra=extra))

    # ==================================================================
    # user-facing API (parity with reference node.py:370-428,702-746)
    # ==================================================================
    def forward_compute(self, tensors=None, **kwargs):
        """Root entry: inject one microbatch into the async pipeline,
        bounded by the in-flight window (parity node.py:370-397)."""
        assert self.node_type == NodeTypes.ROOT or self.fused
        # throttle: in-flight window <= cluster_length
        with self._backward_done:
            while (self.forward_pass_id - self.latest_backward_id
                   > self.cluster_length) and not self._stop.is_set():
                self._backward_done.wait(timeout=1.0)
        if self.reduce_threshold and self.forward_pass_id > 0 and \
                self.forward_pass_id % self.reduce_threshold == 0:
            self.wait_for_backwards()
        fpid = self.forward_pass_id
        self.forward_pass_id += 1
        self._enqueue(1, (str(ActionTypes.ROOT_FORWARD), fpid,
                          {"tensors": tensors, "kwargs": kwargs}))

    def no_grad_forward_compute(self, tensors=None, output_type="val_accuracy",
                                **kwargs):
        assert self.node_type == NodeTypes.ROOT or self.fused
        self.wait_for_backwards()
        fpid = self.eval_pass_id
        self.eval_pass_id += 1
        self._enqueue(1, ("root_no_grad", fpid,
                          {"tensors": tensors, "kwargs": kwargs,
                           "output_type": output_type}))
        if self.fused:
            return None

    def wait_for_backwards(self, timeout: float = 600.0):
        """Block until every injected fpid's backward completed at this
        root (parity node.py:702-710)."""
        if self.node_type != NodeTypes.ROOT and not self.fused:
            return
        deadline = time.monotonic() + timeout
        with self._backward_done:
            while self.latest_backward_id < self.forward_pass_id - 1:
                if self._stop.is_set() or time.monotonic() > deadline:
                    raise TimeoutError(
                        f"rank {self.rank}: pipeline did not drain "
                        f"(fwd={self.forward_pass_id}, "
                        f"bwd={self.latest_backward_id})")
                self._backward_done.wait(timeout=0.5)

    def trigger_save_submodel(self):
        self._handle_save(cascade=True)

    def _forward_stop(self):
        if self.fused or self.comm is None:
            return
        if self.stage + 1 < self.n_stages:
            nxt = self.stage_ranks[self.stage + 1]
            try:
                # queued (not send_sync): must not overtake in-flight
                # forward/eval messages on the same FIFO channel
                self.comm.send(nxt, "fwd", Message(
                    action=ActionTypes.STOP, fpid=0, tensors=[]))
            except KeyError:
                pass

    def stop_cluster(self, timeout: float = 120.0):
        """Root: drain, cascade STOP down the pipeline, stop this node.
        The cascade goes THROUGH the dispatch queue at the lowest priority
        so queued work (e.g. pending eval forwards) runs first — a direct
        send here would overtake it on the FIFO channels."""
        if self.node_type == NodeTypes.ROOT and not self.fused:
            self.wait_for_backwards()
        self._enqueue(3, ("stop_cascade", None, None))
        deadline = time.monotonic() + timeout
        while not self._stop.is_set() and time.monotonic() < deadline:
            time.sleep(0.01)
        self._stop.set()

    def update_with_latest_weights(self, src_rank: int | None = None,
                                   timeout: float = 120.0):
        """Pull the latest parameters over the ctrl channels (parity:
        reference get_latest_weights, communication.py:279-330 /
        node.py:726-730). Equal clusters: full snapshot from one DP
        peer. Unequal clusters: each param-range SEGMENT is pulled from
        a mapped peer of that segment's ring (the reference's multi-peer
        partial restore, node.py:127-135)."""
        if self.comm is None:
            return
        segs = getattr(self.comm, "my_dp_segments", None)
        if segs and src_rank is None:
            named = dict(self.model.named_parameters())
            pulled = 0
            for ranks, _g, names in segs:
                peers = [r for r in ranks if r != self.rank]
                names = [n for n in names if n in named]
                if not peers or not names:
                    continue
                blob = torch.tensor(list("\n".join(names).encode()),
                                    dtype=torch.uint8)
                self.comm.send(peers[0], "ctrl",
                               Message(action=ActionTypes.PREDICTION,
                                       fpid=0, tensors=[(0, blob)],
                                       extra=1))
                tensors = self._weights_reply_q.get(timeout=timeout)
                with torch.no_grad():
                    for i, t in tensors:
                        p = named[names[i]]
                        p.data.copy_(t.to(p.device, p.dtype))
                        pulled += 1
            if pulled:
                self.engine.bump_version()
            return
        if src_rank is None:
            peers = [r for r in self.dp_ranks if r != self.rank]
            if not peers:
                return
            src_rank = peers[0]
        self.comm.send(src_rank, "ctrl",
                       Message(action=ActionTypes.PREDICTION, fpid=0,
                               tensors=[], extra=1))
        tensors = self._weights_reply_q.get(timeout=timeout)
        self.engine.load_param_list([t for _, t in tensors])

    # ==================================================================
    # action handlers
    # ==================================================================
    def _mark_backward_complete(self, fpid: int):
        with self._backward_done:
            self.latest_backward_id = max(self.latest_backward_id, fpid)
            self._backward_done.notify_all()

    def _maybe_reduce(self):
        if not self.reduce_threshold or self.comm is None:
            return
        if self._mem_log and \
                self.engine.n_backwards % self.reduce_threshold == 0:
            # memory telemetry at averaging boundaries (parity: the
            # reference polls NVML around every fwd/bwd,
            # utils.py:211-221 / node.py:447-450; we sample at the much
            # rarer reduce cadence to stay off the hot path)
            from ..utils import gpu_usage
            print(f"[{self.name}] mem {gpu_usage()}", flush=True)
        if getattr(self, "_dp_suspended", False):
            return  # a DP replica is down: skip averaging, keep training
        if self.engine.n_backwards % self.reduce_threshold != 0:
            return
        # The speculative recompute thread swaps param.data to a
        # historical version snapshot while it runs; averaging
        # concurrently would corrupt the snapshot and miss the live
        # weights. Join it first.
        self.engine.join_recompute()
        if getattr(self.comm, "my_dp_segments", None):
            # unequal-cluster DP: per-param-range groups
            average_parameter_segments(
                self.model, self.comm.my_dp_segments,
                self.optimizer, average_optim=self.average_optim)
            self.engine.bump_version()
            return
        if len(self.dp_ranks) > 1:
            if self._reducer is not None:
                # overlapped path: params are frozen until the next
                # optimizer step (reduce_threshold is a multiple of
                # update_frequency), where the hook joins the result
                self._join_reduce()  # drain any straggler first
                params = [p for p in self.model.parameters()]
                tensors = params + _master_tensors(self.optimizer, params)
                if self.average_optim and self.optimizer is not None:
                    for st in self.optimizer.state.values():
                        for k, v in st.items():
                            if k != "master" and isinstance(v, torch.Tensor) \
                                    and v.is_floating_point() and v.numel():
                                tensors.append(v)
                self._reducer.launch(tensors)
                return
            average_parameters(self.model, self.comm.my_dp_group,
                               optimizer=self.optimizer)
            if self.average_optim and self.optimizer is not None:
                average_optimizer_state(self.optimizer, self.comm.my_dp_group)
            self.engine.bump_version()

    def _handle_root_forward(self, fpid: int, payload):
        tensors = payload["tensors"]
        kwargs = payload["kwargs"] or {}
        model_inputs = self._map_model_inputs(tensors, kwargs)
        if self.fused:
            targets = next(self.labels)
            epoch_change = self.labels.take_wrapped()
            args = self._root_args(model_inputs)
            _, stepped, loss = self.engine.find_loss(
                fpid, args, [False] * len(args), targets)
            self.losses.append(loss)
            self._step_scheduler(stepped, epoch_change)
            self._mark_backward_complete(fpid)
            self._maybe_reduce()
            return
        # forward model inputs consumed by later stages
        for name, targets_list in self._model_input_targets.items():
            val = model_inputs.get(name)
            if val is None:
                continue
            by_rank: dict[int, list] = {}
            for (r, gid) in targets_list:
                by_rank.setdefault(r, []).append((gid, val))
            for r, ts in by_rank.items():
                self.comm.send(r, "fwd", Message(
                    action=ActionTypes.FORWARD, fpid=fpid, tensors=ts))
        args = self._root_args(model_inputs)
        outputs = self.engine.forward(fpid, args, self._needs_grad)
        self._send_outputs(ActionTypes.FORWARD, fpid, outputs)

    def _root_args(self, model_inputs: dict) -> list:
        args = []
        for src in self.input_template:
            if src.get("kind") == "model_input":
                v = model_inputs.get(src["name"])
                if torch.is_tensor(v):
                    v = v.to(self.device)
                args.append(v)
            elif src.get("kind") == "const":
                args.append(src.get("value"))
            else:
                raise RuntimeError("root stage with non-model inputs")
        return args

    def _map_model_inputs(self, tensors, kwargs) -> dict:
        mi = {}
        names = self.model_input_names or \
            [s["name"] for s in self.input_template
             if s.get("kind") == "model_input"]
        if tensors is not None and names:
            mi[names[0]] = tensors.to(self.device) \
                if torch.is_tensor(tensors) else tensors
        for k, v in kwargs.items():
            if torch.is_tensor(v):
                v = v.to(self.device)
            mi[k] = v
        return mi

    def _handle_forward(self, fpid: int, payload):
        args = self._build_args(payload["tensors"])
        outputs = self.engine.forward(fpid, args, self._needs_grad)
        self._send_outputs(ActionTypes.FORWARD, fpid, outputs)

    def _step_scheduler(self, stepped: bool, epoch_change: bool):
        """Per-node lr schedule (parity: reference node.py:517-518,
        585-586,603-604): on epoch boundary by default, or after every
        optimizer step when lr_step_on_epoch_change=False."""
        if self.lr_scheduler is None:
            return
        if self.lr_step_on_epoch_change:
            if epoch_change:
                self.lr_scheduler.step()
        elif stepped:
            self.lr_scheduler.step()

    def _handle_find_loss(self, fpid: int, payload):
        args = self._build_args(payload["tensors"])
        targets = next(self.labels)
        epoch_change = self.labels.take_wrapped()
        input_grads, stepped, loss = self.engine.find_loss(
            fpid, args, self._needs_grad, targets)
        self.losses.append(loss)
        self._step_scheduler(stepped, epoch_change)
        self._send_input_grads(fpid, input_grads,
                               extra=1 if epoch_change else 0)
        self._maybe_reduce()

    def _handle_backward(self, fpid: int, payload):
        if isinstance(payload, dict) and "grads" in payload:
            grads, extra = payload["grads"], payload.get("extra", 0)
        else:  # direct-call compatibility (tests)
            grads, extra = payload, 0
        input_grads, stepped = self.engine.backward(fpid, grads)
        self._step_scheduler(stepped, bool(extra & 1))
        if self.node_type != NodeTypes.ROOT:
            self._send_input_grads(fpid, input_grads, extra=extra)
        else:
            self._mark_backward_complete(fpid)
        self._maybe_reduce()

    def _handle_root_no_grad(self, fpid: int, payload):
        tensors = payload["tensors"]
        kwargs = payload["kwargs"] or {}
        output_type = payload.get("output_type", "val_accuracy")
        model_inputs = self._map_model_inputs(tensors, kwargs)
        if self.fused:
            args = self._root_args(model_inputs)
            outputs = self.engine.no_grad_forward(args)
            self._leaf_eval_output(outputs, output_type)
            return
        for name, targets_list in self._model_input_targets.items():
            val = model_inputs.get(name)
            if val is None:
                continue
            by_rank: dict[int, list] = {}
            for (r, gid) in targets_list:
                by_rank.setdefault(r, []).append((gid, val))
            for r, ts in by_rank.items():
                self.comm.send(r, "fwd", Message(
                    action=ActionTypes.NO_GRAD_FORWARD, fpid=fpid, tensors=ts,
                    extra=_OUT_TYPES[output_type]))
        args = self._root_args(model_inputs)
        outputs = self.engine.no_grad_forward(args)
        self._send_outputs(ActionTypes.NO_GRAD_FORWARD, fpid, outputs,
                           extra=_OUT_TYPES[output_type])

    def _handle_no_grad_forward(self, fpid: int, payload):
        args = self._build_args(payload["tensors"])
        outputs = self.engine.no_grad_forward(args)
        if self.node_type == NodeTypes.LEAF:
            self._leaf_eval_output(outputs,
                                   _OUT_TYPES_REV[payload.get("extra", 0)])
        else:
            self._send_outputs(ActionTypes.NO_GRAD_FORWARD, fpid, outputs,
                               extra=payload.get("extra", 0))

    def _leaf_eval_output(self, outputs: tuple, output_type: str):
        out = outputs[0]
        if output_type == "val_accuracy":
            batch = next(self.test_labels)
            if batch is None:
                return
            y = batch[1] if isinstance(batch, (tuple, list)) else batch
            y = y.to(out.device) if torch.is_tensor(y) else y
            pred = out.argmax(dim=-1)
            truth = y.argmax(dim=-1) if torch.is_tensor(y) and y.dim() > 1 \
                else y
            acc = float((pred == truth).float().mean())
            self.val_accuracies.append(acc)
            with open("val_accuracies.txt", "a") as f:
                f.write(f"{round(acc, 4)}\n")
        elif output_type == "accuracy":
            batch = next(self.test_labels)
            if batch is None:
                return
            y = batch[1] if isinstance(batch, (tuple, list)) else batch
            y = y.to(out.device) if torch.is_tensor(y) else y
            pred = out.argmax(dim=-1)
            truth = y.argmax(dim=-1) if torch.is_tensor(y) and y.dim() > 1 \
                else y
            acc = float((pred == truth).float().mean())
            print("Accuracy:", acc)
        else:  # prediction
            torch.save(out.detach().cpu(), "prediction.pt")

    def _template_example_args(self) -> list:
        """Zero-filled example inputs from the plan templates' recorded
        shapes/dtypes (used for the traced submodel export)."""
        args = []
        for src in self.input_template:
            if src.get("kind") == "const":
                args.append(src.get("value"))
            elif src.get("pyscalar"):
                args.append(int(src.get("value", 1)))
            else:
                shape = src.get("shape") or [1]
                dt = _dtype_from_str(src.get("dtype", "torch.float32"))
                args.append(torch.zeros(*shape, dtype=dt,
                                        device=self.device))
        return args

    def _handle_save(self, cascade: bool = False):
        if self.template_path:
            p = Path(self.template_path)
            torch.save(self.model.state_dict(), p / "trained_state_dict.pt")
            # self-contained TorchScript submodel (parity: reference
            # node.py:719-722 saves jit-scripted submodels loadable with
            # NO package; sorter_inference.py:5-21 chains them). Custom
            # autograd ops usually defeat script(), so fall back to an
            # eval-mode trace over the plan-template shapes.
            import os as _os
            tmp = str(p / "submod_script.pt.tmp")
            final = str(p / "submod_script.pt")
            try:
                # script() can COMPILE but still fail at save() on
                # custom-autograd ops — write to a temp and rename only
                # on success so a partial archive never lands
                torch.jit.script(self.model).save(tmp)
                _os.replace(tmp, final)
            except Exception:
                try:
                    was_training = self.model.training
                    self.model.eval()
                    with torch.no_grad():
                        tr = torch.jit.trace(
                            self.model,
                            tuple(self._template_example_args()),
                            check_trace=False)
                    tr.save(tmp)
                    _os.replace(tmp, final)
                    if was_training:
                        self.model.train()
                except Exception as e:
                    print(f"[rank {self.rank}] TorchScript export "
                          f"skipped: {e}", flush=True)
                    if _os.path.exists(tmp):
                        _os.remove(tmp)
        if (cascade or self.node_type != NodeTypes.LEAF) and not self.fused \
                and self.comm is not None and self.stage + 1 < self.n_stages:
            nxt = self.stage_ranks[self.stage + 1]
            try:
                self.comm.send(nxt, "fwd", Message(
                    action=ActionTypes.SAVE_SUBMODEL, fpid=0, tensors=[]))
            except KeyError:
                pass

    def _handle_weights_request(self, payload_src: int, req_tensors=None):
        self._join_reduce()
        if req_tensors:
            # partial pull: request names a contiguous param range
            # (parity: reference get_latest_weights serves name ranges,
            # communication.py:279-330 / endpoints.py:145-154)
            blob = bytes(req_tensors[0][1].to(torch.uint8).tolist())
            names = blob.decode().split("\n")
            self.engine.join_recompute()
            named = dict(self.model.named_parameters())
            tensors = [(i, named[n].detach().clone())
                       for i, n in enumerate(names) if n in named]
        else:
            snap = self.engine.latest_state_snapshot()
            tensors = [(i, t) for i, t in enumerate(snap["params"])]
        self.comm.send(payload_src, "ctrl",
                       Message(action=ActionTypes.PREDICTION, fpid=0,
                               tensors=tensors, extra=2))


class _CommSessionFacade:
    """API-parity shim: the reference exposes
    `node.comm_session.parallel_ring_reduce()` (trainer.py:99,
    communication.py:125); here that is a bucketed RCCL all_reduce on the
    per-stage DP group."""

    def __init__(self, node: Node):
        self.node = node

    def parallel_ring_reduce(self):
        n = self.node
        if n.comm is None:
            return
        n.engine.join_recompute()
        n.join_pending_reduce()
        if getattr(n.comm, "my_dp_segments", None):
            average_parameter_segments(
                n.model, n.comm.my_dp_segments,
                n.optimizer, average_optim=n.average_optim)
            n.engine.bump_version()
            return
        if len(n.dp_ranks) <= 1:
            return
        average_parameters(n.model, n.comm.my_dp_group,
                           optimizer=n.optimizer)
        if n.average_optim and n.optimizer is not None:
            average_optimizer_state(n.optimizer, n.comm.my_dp_group)
        n.engine.bump_version()

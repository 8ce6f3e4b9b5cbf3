"""The ledger of every persistent device buffer, the walker that finds them and the poison that goes into them between steps
(tests/test_gpu_workspace_poison.py poisons and compares; tests/test_workspace_ledger_cpu.py holds the ledger to the source).

The training step, the drop-in flow and the inference path live on workspaces that outlast a call. After the first step the rows
off a work list hold what an earlier step left there: finite, plausible values. A launch that reads one gives a slightly wrong
number, not a NaN, and no operator suite (fresh NaN-filled buffers, one launch) can see it. The contract, stated once per buffer:

  rewritten  every element a launch of this step reads was written earlier in the same step, or is never read.
             Poison: all-ones bytes (NaN in f32 / bf16 / f64, 0xFF in the 1-bit ReLU masks) - unless a consumer derives an address,
             a bin or a trip count from the values, or the buffer is an integer list: then finite / in-range poison, and the row says so.
  masked     rows off this step's work lists are not written and MAY be read, but only under an exact zero factor or a select (the
             row cites the line). Poison: the buffer's own contents after the clean arm's same step, shuffled across rows - a stale
             row by construction.
  state      carried across steps by design (parameters, moments, weight images, counters, static inputs of captured graphs,
             references to the caller's tensors). Not poisoned; the row names the owner.
  const      written once (tables, maps, constants). Not poisoned.

`walk(roots)` finds every device tensor reachable from the given objects - through attributes of the package's own objects and of
nn.Modules, dicts, lists and tuples - once per (storage, offset, shape, stride). `classify` gives each the FIRST ledger row whose
pattern (fnmatch on the dotted path) matches, and fails on a tensor no row names: a buffer added later has to be classified before
the suite passes.

Safety of the poison: a stale read must show as a wrong number, never as a wrong address. Integer buffers only get values their
consumer accepts (indices in [0, capacity), counts in [0, capacity]); float buffers whose values steer a search get finite stale
values; descriptor tables (raw device addresses in uint8 tensors) are `const` and never written; every write goes through the tensor
the walker found."""
import fnmatch
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "vdn-nerf_amd")
for _p in (PKG, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

CLASSES = ("rewritten", "masked", "state", "const")
POISONED = ("rewritten", "masked")
_OWN = ("vdn_hip", "dpt_models", "vdn_train")


# ------------------------------------------------------------------------------------------------------------------------
# the ledger. Row: (pattern, class, poison, citation / owner). First match wins, so the specific rows stand in front.
# poison: "ones" | "stale" | ("index", capacity) | ("count", capacity) | None (state / const); capacity = a function of the owning
# TrainEngine. Citations are file:line of the line that justifies the class (vdn-nerf_amd/ paths are given from the package root).
# ------------------------------------------------------------------------------------------------------------------------
_P = lambda e: e.P           # rows of the foreground planes
_Q = lambda e: e.Q           # rows of the background planes
_N = lambda e: e.N           # inside samples per ray
_T = lambda e: e.T           # all samples per ray

# keys of TrainEngine.w (vdn_hip/train.py) -> (class, poison, citation). The CPU test reads the keys assigned in the source and
# wants each of them here.
W_LEDGER = {
    # ---- step preparation: vdn_train_prep / vdn_sections / vdn_merge_sorted write every element of the batch (train.py:636-668)
    "dists": ("rewritten", "ones", "train.py:645 vdn_train_prep writes all [B,N] sections before the compositor reads them"),
    "mid_z": ("rewritten", "ones", "train.py:645 (a slot of the output arena) all [B,N] mid-points written by the preparation"),
    "z_feed": ("rewritten", "ones", "train.py:639 merged depths of all [B,T], written by the preparation"),
    "bg_dists": ("rewritten", "ones", "train.py:645"),
    "bg_mid": ("rewritten", "ones", "train.py:645 (arena slot)"),
    # ---- work lists: int32, poisoned in range only
    "fg_active.0": ("rewritten", ("index", _P), "train.py:647 rows [0, n) written by the preparation; consumers stop at n. In-range: an index"),
    "fg_active.1": ("rewritten", ("count", _P), "train.py:647 / 663 written every step (a view of _fg_cnt). In-range: a row count"),
    "fg_active.2": ("rewritten", ("count", _N), "train.py:647 per-ray counts, written every step. In-range: a count of samples of a ray"),
    "fg_inner": ("rewritten", ("count", _P), "train.py:642 / 663 rows of the first class and the heads' rows (views of _fg_cnt)"),
    "bg_active.0": ("rewritten", ("index", _Q), "train.py:648 as fg_active.0"),
    "bg_active.1": ("rewritten", ("count", _Q), "train.py:648 / 683"),
    "bg_active.2": ("rewritten", ("count", _T), "train.py:648 per-ray counts"),
    "fg_rest.0": ("rewritten", ("index", _P), "train.py:824 the list's complement, written by vdn_foreground_active(complement=1)"),
    "fg_rest.1": ("rewritten", ("count", _P), "train.py:824"),
    "fg_rest.2": ("rewritten", ("count", _N), "train.py:824"),
    # ---- dense per-point outputs: the compositor reads every sample and multiplies the ones off the lists by exact zeros
    "sdf": ("masked", "stale", "train.py:403-404, 417: rows off the foreground list keep old values; csrc/k_composite_row.h:67 reads them, :88 al * inside"),
    "normals": ("masked", "stale", "train.py:403-404 (arena slot): as sdf, csrc/k_composite_row.h:68"),
    "bg_density": ("masked", "stale", "train.py:445-446: points the background list skips are read and weighted (1 - inside) = 0, csrc/k_composite_row.h:63, 88"),
    "bg_rgb": ("masked", "stale", "train.py:445-446, csrc/k_composite_row.h:89-91"),
    "bg_feat": ("masked", "stale", "train.py:447, csrc/k_composite_row.h:170 feat_mix"),
    # ... but the heads' outputs behind their prefix are NOT read: a select stands in front of the load (torch.zeros all the same)
    "col_out": ("rewritten", "ones", "train.py:429 torch.zeros, yet csrc/k_composite_row.h:84-85 loads the colour only where |p| < 1 - the rows the head wrote"),
    "vdn_out": ("rewritten", "ones", "train.py:431 torch.zeros, yet csrc/k_composite_row.h:155 feat_load reads the foreground feature only where inside != 0"),
    # ---- saves of the forwards, in list order: written on rows [0, n), read by the chains and the GEMM on rows [0, n)
    "feat": ("rewritten", "ones", "train.py:417 torch.empty: feature plane of the listed rows, read by the heads / GEMM on those rows"),
    "H": ("rewritten", "ones", "train.py:423 torch.empty: saved on listed rows, the GEMM contracts over P_dev rows (train.py:513)"),
    "V": ("rewritten", "ones", "train.py:423"),
    "PE": ("rewritten", "ones", "train.py:423"),
    "S": ("rewritten", "ones", "train.py:425 fp32 softplus' planes"),
    "S_rest": ("rewritten", "ones", "train.py:829 scratch of the inference launch on the complement"),
    "col_h": ("rewritten", "ones", "train.py:429 torch.zeros, but rows behind the heads' prefix are read by no kernel (DwGroup.cap, train.py:540)"),
    "col_small": ("rewritten", "ones", "train.py:429"),
    "vdn_h": ("rewritten", "ones", "train.py:431"),
    "vdn_small": ("rewritten", "ones", "train.py:431"),
    "col_extra": ("rewritten", "ones", "train.py:433"),
    "col_mask": ("rewritten", "ones", "train.py:440 1-bit ReLU masks: written by the head's forward on its rows, read on its rows"),
    "vdn_mask": ("rewritten", "ones", "train.py:442"),
    "nf_h": ("rewritten", "ones", "train.py:450 torch.empty: background saves in compact order (train.py:677)"),
    "nf_pe": ("rewritten", "ones", "train.py:450"),
    "nf_feature": ("rewritten", "ones", "train.py:450"),
    "nf_vpe": ("rewritten", "ones", "train.py:450"),
    "nf_hv": ("rewritten", "ones", "train.py:450"),
    "nf_mask": ("rewritten", "ones", "train.py:451"),
    "nf_mask_v": ("rewritten", "ones", "train.py:451"),
    # ---- per-ray outputs of the compositor (arena slots and alpha): every ray written
    "weights": ("rewritten", "ones", "train.py:727 compositor writes all [B,T]"),
    "alpha": ("rewritten", "ones", "train.py:727"),
    "cdf": ("rewritten", "ones", "train.py:727"),
    "inside": ("rewritten", "ones", "train.py:727"),
    "color": ("rewritten", "ones", "train.py:728"),
    "wsum": ("rewritten", "ones", "train.py:728"),
    "wmax": ("rewritten", "ones", "train.py:728"),
    "s_val": ("rewritten", "ones", "train.py:728"),
    "eik_partial": ("rewritten", "ones", "train.py:729 per-ray sums, reduced by vdn_eikonal_reduce in the same step"),
    "eik": ("rewritten", "ones", "train.py:729"),
    "feat_out": ("rewritten", "ones", "train.py:731"),
    # ---- backward intermediates
    "d_sdf": ("rewritten", "ones", "train.py:971 torch.empty: the compositor's adjoint writes every sample; the SDF chains read listed rows"),
    "d_normals": ("rewritten", "ones", "train.py:971 written by the compositor's adjoint for every sample, then accumulated into"),
    "d_color": ("rewritten", "ones", "train.py:971"),
    "d_featvec": ("rewritten", "ones", "train.py:1075-1077 the first head overwrites rows [0, n_rows_all)"),
    "d_vdn": ("rewritten", "ones", "train.py:973-976 written by the adjoint, or zeroed"),
    "feat_scratch": ("rewritten", "ones", "train.py:974 scratch inside the adjoint's launches"),
    "d_var_partial": ("rewritten", "ones", "train.py:983 per-ray partials, summed by the finalize launch"),
    "d_variance": ("rewritten", "ones", "train.py:460 allocated, used by no launch"),
    "col_dout": ("rewritten", "ones", "train.py:461 torch.zeros, rows behind the heads' prefix read by no kernel (DwGroup.cap)"),
    "col_dh": ("rewritten", "ones", "train.py:461"),
    "vdn_dout": ("rewritten", "ones", "train.py:463"),
    "vdn_dh": ("rewritten", "ones", "train.py:463"),
    "UB": ("rewritten", "ones", "train.py:464 torch.empty: written by the rbar chain on listed rows"),
    "EX": ("rewritten", "ones", "train.py:464"),
    "AB": ("rewritten", "ones", "train.py:464"),
    "d_bg_density": ("rewritten", "ones", "train.py:466 the adjoint writes every background sample"),
    "d_bg_rgb": ("rewritten", "ones", "train.py:466"),
    "d_bg_feat": ("rewritten", "ones", "train.py:467, 980-982"),
    "nf_do": ("rewritten", "ones", "train.py:468 deltas of the background network's backward, compact order"),
    "nf_dv": ("rewritten", "ones", "train.py:468"),
    "nf_dhead": ("rewritten", "ones", "train.py:468"),
    "nf_dh": ("rewritten", "ones", "train.py:468"),
    # ---- ray adjoints (train.py:558-563), allocated by the first pose step
    "U_pe": ("rewritten", "ones", "train.py:843 written by the SDF forward on listed rows, read by fbar on listed rows"),
    "d_pts": ("rewritten", "ones", "train.py:1082 zeroed every pose step, then written on listed rows"),
    "d_dirs": ("rewritten", "ones", "train.py:1083"),
    "d_dists": ("rewritten", "ones", "train.py:985 written by the compositor's adjoint"),
    "d_dir_cos": ("rewritten", "ones", "train.py:985"),
    "d_rays_o": ("rewritten", "ones", "train.py:1139 written by vdn_ray_adjoint"),
    "d_rays_d": ("rewritten", "ones", "train.py:1139"),
    "d_z": ("rewritten", "ones", "train.py:1139"),
    "d_bg_pts": ("rewritten", "ones", "train.py:1040 zeroed every pose step"),
    "d_bg_dirs": ("rewritten", "ones", "train.py:1041"),
    "d_bg_dists": ("rewritten", "ones", "train.py:987"),
    "d_z_out": ("rewritten", "ones", "train.py:1138"),
}

# attributes of Trainer (vdn_train/trainer.py) that hold device tensors -> (class, poison, citation)
TRAINER_LEDGER = {
    "_param_flat": ("state", None, "Trainer: the parameters (trainer.py:99)"),
    "_exp_avg": ("state", None, "Trainer: Adam's first moments (trainer.py:107)"),
    "_exp_avg_sq": ("state", None, "Trainer: Adam's second moments (trainer.py:108)"),
    "_eik_global": ("rewritten", "ones", "trainer.py:701 written by vdn_eikonal_terms (data-parallel steps only)"),
    "_eik_partial": ("rewritten", "ones", "trainer.py:701"),
    "g_color": ("rewritten", "ones", "trainer.py:508 / 543 written by the loss launch or the fused compositor before the backward reads it"),
    "g_weights": ("rewritten", "ones", "trainer.py:545 written by the loss launch when the mask loss is on, else handed to nobody"),
    "g_eik": ("rewritten", "ones", "trainer.py:543"),
    "scalars": ("rewritten", "ones", "trainer.py:543 the six scalars, written by the loss launch every step"),
    "g_feats": ("rewritten", "ones", "trainer.py:516 / 547 written when the depth term is on, else handed to nobody"),
    "bg": ("const", None, "trainer.py:171 the white background"),
    "_jitter": ("state", None, "Trainer: the jitter pool of the next 32 steps (trainer.py:472)"),
    "_fg_cnt_g": ("rewritten", ("count", _P), "trainer.py:691 data-parallel steps only"),
    "_g_log.*": ("rewritten", "ones", "trainer.py:561 scratch copies the logging launch writes"),
    # ---- learnable cameras (_init_cameras)
    "_pose_flat": ("state", None, "Trainer: the flat pose buffer (trainer.py:188)"),
    "_pose_grad": ("rewritten", "ones", "trainer.py:259 vdn_pose_adjoint writes the dense gradient of every camera before Adam reads it"),
    "_pose_exp_avg": ("state", None, "Trainer: pose moments (trainer.py:194)"),
    "_pose_exp_avg_sq": ("state", None, "Trainer: pose moments (trainer.py:195)"),
    "_rows": ("rewritten", "stale", "trainer.py:238 vdn_gen_rays_pose writes every row. Finite poison: rays and near / far feed the sampler's search"),
    "_near": ("rewritten", "stale", "trainer.py:238. Finite in-range poison: the sampler's inverse-CDF search runs between near and far"),
    "_far": ("rewritten", "stale", "trainer.py:238"),
    "_init_c2w": ("const", None, "trainer.py:208 initial cameras"),
    "_intrin_inv": ("const", None, "trainer.py:213 K^-1, rebuilt only by a checkpoint load"),
    "_pose_scratch": ("rewritten", "ones", "trainer.py:262 f64 partials inside vdn_pose_adjoint"),
    "_last_pixels.*": ("state", None, "the caller: pixel coordinates of the last step, held by reference (trainer.py:241)"),
}

# attributes of TrainEngine / DwGroup / _Net outside w
ENGINE_LEDGER = {
    "_out_arena": ("rewritten", "ones", "train.py:415 the slots are classified on their own (w.*); the 64-element padding between them is read by nobody"),
    "_fg_cnt": ("rewritten", ("count", _P), "train.py:420 [listed, first class, heads' rows, pad]: written by the preparation or filled with P (663)"),
    "_grad_flat": ("state", None, "TrainEngine: the flat gradient (train.py:473). No finalize descriptor accumulates (train.py:222) and every network with "
                   "weight-gradient entries has its slice overwritten each step - NaN between steps changes nothing, "
                   "test_flat_gradient_is_overwritten_where_a_network_has_entries - but a renderer with n_outside = 0 has no entries for "
                   "the background network: that slice keeps the zeros of its allocation for good"),
    "slab": ("rewritten", "ones", "train.py:506 torch.empty: every split the finalize sums was written by this step's GEMM"),
    "colsum": ("rewritten", "ones", "train.py:507"),
    "maps": ("const", None, "train.py:505 row / column maps of the weight-gradient plan"),
    "_var_map": ("const", None, "train.py:519 the one-row map of the variance's finalize descriptor"),
    "dweff": ("rewritten", "ones", "train.py:80 d W_eff: finalize writes every matrix view before the weight-norm backward reads it; gaps are read by nobody"),
}
DWGROUP_LEDGER = {
    "dw": ("const", None, "train.py:322 GEMM descriptors: raw device addresses, uploaded once - never written"),
    "fin": ("const", None, "train.py:325 finalize descriptors"),
    "wn": ("const", None, "train.py:326 weight-norm descriptors"),
    "cap.0": ("rewritten", ("count", _P), "train.py:540 a view of _fg_cnt"),
}

LEDGER = []


def _rows(prefix, table):
    for key, (cls, poison, cite) in table.items():
        LEDGER.append((prefix + key, cls, poison, cite))


# references to tensors of the last call (the caller's inputs, allocations of the last forward): not workspaces. They stand in front
# of everything, since they alias what other paths also reach.
LEDGER += [
    ("*._ctx.*", "state", None, "the caller / the allocator: inputs and depths of the last forward, by reference (train.py:733)"),
    ("*._fwd_rays.*", "state", None, "the caller: rays of the last forward (train.py:593)"),
    ("*._bwd_args_keep.*", "state", None, "the caller: adjoints the compositor's argument block points at (train.py:988)"),
    ("*._fused_keep.*", "state", None, "the caller: inputs of the fused compositor's launch (train.py:749)"),
    ("*._bwd_train.*", "state", None, "the caller: the fused loss' inputs (train.py:746)"),
    ("*._car_dev", "state", None, "a graph plan's annealing ratio (train.py:592)"),
    ("*._pending_merge.*", "state", None, "the allocator: the sampler's last round, consumed by the same step's preparation (renderer.py:480)"),
    ("*.last_eikonal_terms", "state", None, "the caller: a view of the last render()'s outputs (renderer.py:691)"),
    ("*._grad_list.*", "state", None, "views of the flat gradient: as _grad_flat (train.py:1174)"),
]
_rows("*.w.", W_LEDGER)
_rows("*.groups.*.", DWGROUP_LEDGER)
_rows("*.nets.*.", {"dweff": ENGINE_LEDGER["dweff"]})
_rows("*.", {k: v for k, v in ENGINE_LEDGER.items() if k != "dweff"})
_rows("tr.", TRAINER_LEDGER)
LEDGER += [
    ("*.grad_views.*", "state", None, "views of the flat gradient: as _grad_flat (train.py:476)"),
    ("*.grads.*", "state", None, "views of the flat gradient: as _grad_flat (train.py:85)"),
    # ---- graph plans of render() under grad (dpt_models/renderer.py: _TrainPlan)
    ("*._plans.*.state.*", "state", None, "a graph plan's copy of PLAN_STATE: references (renderer.py:256)"),
    ("*._plans.*.bwd.*", "state", None, "static adjoint inputs of a captured backward, staged before every replay (renderer.py:287, 301)"),
    ("*._plans.*.z", "state", None, "a captured forward's sampler output inside the graph's private pool (renderer.py:255)"),
    ("*._plans.*.z_out", "state", None, "as z: inside the captured forward's private pool (renderer.py:255)"),
    ("*._plans.*.*", "state", None, "static inputs of a captured forward, staged before every replay (renderer.py:239-247, 266)"),
    # ---- the renderer and its networks
    ("*._const_cache.*", "const", None, "renderer.py:380-389 linspace tables"),
    ("*._jitter.*", "state", None, "the renderer: jitter pool of the next 16 batches (renderer.py:427)"),
    ("*._shade_ticket", "state", None, "the renderer: ticket counter of the fused shading launch, back at zero after every launch (renderer.py:656)"),
    ("*._scratch.*", "masked", "stale", "fields.py:511-521: rows off the background list keep an earlier call's outputs; render_core multiplies them by zero"),
    ("*._img_tables.*", "const", None, "images.py refresh_together: descriptor tables of the image build"),
    ("*._img_cache.*", "const", None, "trainer.py:355 descriptor tables of the image build"),
    ("*._img.*", "state", None, "the network: weight images, bf16 blobs, inverse norms (images.py NetImages), rebuilt from the parameters when they change"),
    ("*.img.*", "state", None, "as _img (the engine's reference, train.py:79)"),
    ("*._pt_plans.*.maps", "const", None, "points.py:59 row / column maps"),
    ("*._pt_plans.*.group.*", "const", None, "points.py:74 descriptor tables"),
    ("*._parameters.*", "state", None, "the module: parameters (views of the Trainer's flat buffer once it exists)"),
    ("*._buffers.*", "const", None, "the module: registered buffers"),
    ("*.params.*", "state", None, "the parameters, by reference (train.py:471)"),
    ("*._params.*", "state", None, "the parameters, by reference (trainer.py:97)"),
    # ---- cameras of the learnable-pose Trainer
    ("*.pose_net.*", "state", None, "LearnPose: r / t are views of the flat pose buffer; init_c2w is its constant"),
    ("*.intrin_net.*", "state", None, "LearnIntrin: its parameters"),
    ("tr.cameras.*", "const", None, "the resident images, pixels and cameras of the scene (vdn_train/rays.py)"),
    ("tr._pixels.*", "const", None, "as tr.cameras"),
]


# ------------------------------------------------------------------------------------------------------------------------
# the walker
# ------------------------------------------------------------------------------------------------------------------------
def _key_name(k):
    """A dict key as a path element: strings as they are; of a tuple key (an engine's or a plan's) the small scalars - addresses
    and ids, which differ from run to run, are left out."""
    if isinstance(k, str):
        return k
    if isinstance(k, bool) or k is None:
        return str(k)
    if isinstance(k, (int, float)):
        return repr(k) if abs(k) < (1 << 20) else "#"
    if isinstance(k, tuple):
        parts = [_key_name(x) for x in k if isinstance(x, (str, int, float, bool)) and not (isinstance(x, int) and not isinstance(x, bool) and abs(x) >= (1 << 20))]
        return "-".join(parts) if parts else "#"
    return type(k).__name__


class Found:
    """One tensor the walker found: `name` the first path that reached it, `aliases` the later ones, `engine` the nearest
    TrainEngine above it (its shapes give the capacities of integer poison)."""

    def __init__(self, name, tensor, engine):
        self.name, self.tensor, self.engine, self.aliases = name, tensor, engine, []
        self.row = None

    @property
    def span(self):
        """(storage address, first byte, one past the last byte) of the elements the tensor can reach."""
        t = self.tensor
        es = t.element_size()
        lo = t.storage_offset() * es
        n = 0 if t.numel() == 0 else 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
        return t.untyped_storage().data_ptr(), lo, lo + n * es


def walk(roots, device_only=True):
    """roots: {name: object} in order -> [Found] in discovery order, one per distinct (storage, offset, shape, stride)."""
    seen_obj, seen_t, out = set(), {}, []

    def visit(obj, name, eng):
        if isinstance(obj, torch.Tensor):
            if device_only and obj.device.type == "cpu":
                return
            key = (obj.untyped_storage().data_ptr(), obj.storage_offset(), tuple(obj.shape), tuple(obj.stride()), obj.dtype)
            if key in seen_t:
                seen_t[key].aliases.append(name)
            else:
                seen_t[key] = f = Found(name, obj, eng)
                out.append(f)
            g = getattr(obj, "grad", None) if obj.is_leaf else None
            if g is not None:
                visit(g, name + ".grad", eng)
            return
        if obj is None or isinstance(obj, (str, bytes, int, float, bool, complex)):
            return
        if id(obj) in seen_obj:
            return
        if isinstance(obj, dict):
            seen_obj.add(id(obj))
            used = {}
            for k, v in list(obj.items()):
                kn = _key_name(k)
                used[kn] = used.get(kn, 0) + 1
                if used[kn] > 1:
                    kn = "%s~%d" % (kn, used[kn])
                visit(v, name + "." + kn, eng)
            return
        if isinstance(obj, (list, tuple)):
            seen_obj.add(id(obj))
            for i, v in enumerate(obj):
                visit(v, "%s.%d" % (name, i), eng)
            return
        mod = type(obj).__module__ or ""
        if isinstance(obj, torch.nn.Module) or mod.split(".")[0] in _OWN:
            if not hasattr(obj, "__dict__"):
                return
            seen_obj.add(id(obj))
            if type(obj).__name__ == "TrainEngine":
                eng = obj
            for k, v in list(vars(obj).items()):
                visit(v, name + "." + k, eng)

    for name, obj in roots.items():
        visit(obj, name, None)
    return out


# rows that name a REFERENCE to a tensor somebody else owns: when the owner's path reaches the tensor too, that path classifies it
REFERENCES = ("*._ctx.*", "*._fwd_rays.*", "*._bwd_args_keep.*", "*._fused_keep.*", "*._bwd_train.*", "*._car_dev", "*._pending_merge.*",
              "*.last_eikonal_terms", "*._grad_list.*", "*.grad_views.*", "*.grads.*", "*._plans.*.state.*", "*.params.*", "*._params.*")


def _is_reference(row):
    return row is not None and row[0] in REFERENCES


def classify(found, ledger=None):
    """Give every Found its ledger row: the first row that matches its name. A tensor first reached through a reference (an
    engine's _ctx, a plan's state ...) and later through its owner takes the owner's path as its name and the owner's row.
    AssertionError listing the tensors no row names."""
    ledger = LEDGER if ledger is None else ledger
    match = lambda name: next((r for r in ledger if fnmatch.fnmatchcase(name, r[0])), None)
    missing = []
    for f in found:
        names = [f.name] + f.aliases
        rows = [match(n) for n in names]
        pick = next((i for i, r in enumerate(rows) if r is not None and not _is_reference(r)), None)
        if pick is None:
            pick = next((i for i, r in enumerate(rows) if r is not None), None)
        if pick is None:
            missing.append("%s %s %s" % (f.name, tuple(f.tensor.shape), f.tensor.dtype))
            continue
        if pick:
            names[0], names[pick] = names[pick], names[0]
            f.name, f.aliases = names[0], names[1:]
        f.row = rows[pick]
        assert f.row[1] in CLASSES, f.row
    assert not missing, "persistent device tensors without a ledger row (tests/poison.py):\n  " + "\n  ".join(missing)
    return found


# ------------------------------------------------------------------------------------------------------------------------
# poison generators (any device; tests/test_workspace_ledger_cpu.py runs them on CPU tensors)
# ------------------------------------------------------------------------------------------------------------------------
def ones_bytes_(t):
    """All-ones bytes into every element of t: NaN for f32 / bf16 / f16 / f64, 0xFF for uint8."""
    assert t.dtype in (torch.float32, torch.bfloat16, torch.float16, torch.float64, torch.uint8), t.dtype
    if t.numel() == 0:
        return t
    if t.is_contiguous():
        t.reshape(-1).view(torch.uint8).fill_(255)
    else:
        pat = torch.full((t.element_size(),), 255, dtype=torch.uint8, device=t.device).view(t.dtype)
        t.copy_(pat.expand(t.shape) if t.dim() else pat.reshape(()))
    return t


def int_range(kind, capacity):
    """[lo, hi] (inclusive) of integer poison: an index of a buffer of `capacity` rows, or a count of them. Capacity 0 has no valid
    index: the consumer then reads none, and 0 is written."""
    assert kind in ("index", "count") and capacity >= 0
    return (0, max(capacity - 1, 0)) if kind == "index" else (0, capacity)


def int_poison_(t, kind, capacity, gen):
    assert t.dtype in (torch.int32, torch.int64), t.dtype
    lo, hi = int_range(kind, capacity)
    vals = torch.randint(lo, hi + 1, tuple(t.shape), generator=gen, dtype=torch.int64).to(device=t.device, dtype=t.dtype)
    t.copy_(vals)
    return t


def shuffled_stale(src, gen):
    """A permutation of src's contents across rows: chunks of the last dimension (single elements of a 1-D tensor) change places."""
    flat = src.reshape(-1)
    g = src.shape[-1] if src.dim() >= 2 else 1
    if flat.numel() == 0:
        return src.clone()
    rows = flat.view(-1, g)
    perm = torch.randperm(rows.shape[0], generator=gen).to(src.device)
    return rows[perm].reshape(src.shape).contiguous()


def generator(seed):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed)
    return g


# ------------------------------------------------------------------------------------------------------------------------
# applying it
# ------------------------------------------------------------------------------------------------------------------------
def snapshot_stale_sources(found):
    """{name: clone} of every buffer whose poison is "stale" (the clean arm calls this behind every step)."""
    return {f.name: f.tensor.detach().clone() for f in found if f.row[2] == "stale"}


def apply(found, stale=None, seed=0, only=None, override=None):
    """Poison every `rewritten` and `masked` tensor of `found` (classified). stale: {name: tensor} the clean arm's contents after
    the same step. only: a set of names to restrict to (narrowing). override: {name: poison} replacing a row's poison (the bite
    checks; a state / const tensor named here is poisoned too). Containers go first (largest span of a storage first), so a slot's own class has the last word.
    -> {name: (class, poison kind, bytes)} of what was written."""
    gen = generator(seed)
    todo = [f for f in found if (f.row[1] in POISONED or f.name in (override or {})) and (only is None or f.name in only)]
    todo.sort(key=lambda f: -(f.span[2] - f.span[1]))
    done = {}
    with torch.no_grad():
        for f in todo:
            t = f.tensor.detach()
            poison = (override or {}).get(f.name, f.row[2])
            if poison == "ones":
                ones_bytes_(t)
                kind = "ones"
            elif poison == "stale":
                src = None if stale is None else stale.get(f.name)
                if src is None:
                    # a buffer that did not exist behind the clean arm's step (allocated lazily later): its own contents
                    src = t.clone()
                assert src.shape == t.shape and src.dtype == t.dtype, (f.name, src.shape, t.shape)
                t.copy_(shuffled_stale(src, gen))
                kind = "stale"
            else:
                kind, cap = poison
                assert f.engine is not None, f.name
                int_poison_(t, kind, int(cap(f.engine)), gen)
            done[f.name] = (f.row[1], kind, f.span[2] - f.span[1])
    return done


# ------------------------------------------------------------------------------------------------------------------------
# coverage
# ------------------------------------------------------------------------------------------------------------------------
def _union(iv):
    out = []
    for lo, hi in sorted(iv):
        if out and lo <= out[-1][1]:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return out


def _minus(a, b):
    """Measure of union(a) outside union(b)."""
    a, b = _union(a), _union(b)
    total = 0
    for lo, hi in a:
        cur = lo
        for blo, bhi in b:
            if bhi <= cur or blo >= hi:
                continue
            if blo > cur:
                total += blo - cur
            cur = max(cur, bhi)
        if cur < hi:
            total += hi - cur
    return total


def coverage(found, done):
    """-> dict(classes={class: (tensors, bytes)}, non_state_bytes, poisoned_bytes, clobbered): bytes are measured per storage on
    the union of the tensors' spans, so views count once. non_state_bytes: reachable bytes outside every state / const tensor;
    poisoned_bytes: those of them a poisoned tensor covers; clobbered: bytes of state / const tensors a poison write also covered
    (must be 0)."""
    per = {}
    classes = {c: [0, 0] for c in CLASSES}
    for f in found:
        st, lo, hi = f.span
        d = per.setdefault(st, {"all": [], "keep": [], "hit": []})
        d["all"].append((lo, hi))
        if f.row[1] in POISONED:
            if f.name in done:
                d["hit"].append((lo, hi))
        else:
            d["keep"].append((lo, hi))
        classes[f.row[1]][0] += 1
    for c in CLASSES:
        by = {}
        for f in found:
            if f.row[1] == c:
                by.setdefault(f.span[0], []).append(f.span[1:])
        classes[c][1] = sum(_minus(iv, []) for iv in by.values())
    non_state = sum(_minus(d["all"], d["keep"]) for d in per.values())
    missed = sum(_minus(d["all"], d["keep"] + d["hit"]) for d in per.values())
    clobbered = sum(_minus(d["keep"], []) - _minus(d["keep"], d["hit"]) for d in per.values())
    return dict(classes={c: tuple(v) for c, v in classes.items()}, non_state_bytes=non_state, poisoned_bytes=non_state - missed,
                clobbered=clobbered)


def poison_free_blocks_(device):
    """All-ones bytes into every block torch's caching allocator holds free on `device`: what the next torch.empty of a call gets.
    For code whose per-call buffers are float planes no address is derived from (vdn_hip/points.py: saves and deltas of the
    standalone networks). -> (blocks, bytes)."""
    torch.cuda.synchronize(device)
    idx = torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device()
    sizes = sorted((b["size"] for seg in torch.cuda.memory_snapshot() if seg["device"] == idx for b in seg["blocks"] if b["state"] == "inactive"),
                   reverse=True)
    held = [torch.empty(s, dtype=torch.uint8, device=device) for s in sizes if s >= 512]      # (largest first: each takes its own block)
    for t in held:
        t.fill_(255)
    total = sum(t.numel() for t in held)
    del held
    torch.cuda.synchronize(device)
    return len(sizes), total


def roots_of(tr=None, rend=None):
    """The roots of a walk, renderer first (its networks name the parameters), then the Trainer (its engine, groups and pose buffers)."""
    roots = {}
    if rend is None and tr is not None:
        rend = tr.r
    if rend is not None:
        roots["rend"] = rend
    if tr is not None:
        roots["tr"] = tr
    return roots

"""Muon: momentum orthogonalised by a Newton-Schulz iteration, inside the captured update.

Every orthogonalised tensor (``ortho="conv"``: every 4-D parameter; or an iterable of parameters)
is viewed as a matrix ``[K][rest]`` and takes, all scalars fp32, ``fma`` = one rounding, ``gs`` =
``grad_scale`` (times the clip coefficient under the gradient guard):

    G  = g * gs
    m' = fma(mu, m, G)
    d  = fma(mu, m', G) if nesterov else m'
    S  = sum d^2 ;  s0 = 1 / (sqrt(S) + 1e-7)         S from fp32 chunk partials, fixed order
    X0 = bf16(d)                                      the iteration runs on X0 s0 (see below)
    5 times:  A = bf16(X X^T);  B = bf16(fma(b, A, c * (A A)));  X = bf16(fma(a, X, B X))
              (a, b, c) = (3.4445, -4.7750, 2.0315) as fp32
    p' = fma(-(lr * s), O, fma(-(lr * wd), p, p))     O = X5,  s = fp32(sqrt(max(1, rows / cols)))

with ``rows = K`` and ``cols = numel / K``. ``mu`` defaults to 0.95 and nesterov to True, ``wd``
honours the ``no_decay`` mask, every GEMM accumulates in fp32 and the bf16 roundings shown are
the only ones. The normalisation is no pass of its own: the start stays ``bf16(d)``, unscaled,
and the first iteration carries ``s0`` in its scalars,

    A0 = bf16((s0 * s0) * (X0 X0^T))
    B0 = bf16(fma(b, A0, c * (A0 A0)))
    X1 = bf16(fma(a * s0, X0, s0 * (B0 X0)))

which is the iteration on ``X0 s0`` with the start's one bf16 rounding taken on ``d`` instead of
on ``d s0``; every later iteration is the plain one. Every other tensor (biases, BatchNorm
vectors, ``fc``) takes FusedSGD's momentum rule as it is, in the same launch, with the same
learning rate, momentum and nesterov setting.

Orientation and padding. The staged matrix is always wide: if ``K > numel / K`` (ResNet's 1x1
expansion convs, VGG's 64 x 27 input conv) the transpose is staged, and O is read back through
the transposed index. Both dimensions are zero-padded to multiples of 32, the GEMM's tile; zero
rows and columns stay zero through the iteration, so this is exact. The column order is whatever
the master's arena layout has (ops/common.py ``weight_krsc``: [K][R][S][C] on the GPU): the
orthogonalisation commutes with a column permutation, so nothing is re-laid. It commutes as
mathematics and in every store point of the rule; the bits of O are those of a permuted input only
up to the order of the GEMMs' fp32 sums, which the permutation changes (``X X^T`` for a wide
tensor, ``A A`` and ``B X`` for a tall one). tests/test_muon_cpu.py checks the bitwise statement
with a matmul whose sums do not depend on their order, not with ``_cpu_step``'s ``torch.matmul``.

GPU (csrc/kernels/muon.hip, api.h MuonStage / MuonGemm / MuonArgs): the stage launch writes
``bf16(d)`` and the chunk partials of ``sum d^2``; three grouped GEMM launches per iteration run
every tensor's product of one kind in one dispatch; the MUON items of ``sgd_pack_kernel`` form
``m'`` again from the stage kernel's own device function, read O and apply the last line. 17
launches more than SGD for any number of tensors. The staging buffers (two X matrices, A and B
per tensor, bf16) are allocated once and zeroed once, their addresses are baked into the tables,
and a captured step replays them unchanged. Launch order with the gradient guard: sum of
squares, stage (which takes the clip coefficient from the guard's partials), the GEMMs, the
update. A step the guard skips changes no ``m``, ``p`` or EMA.

It refuses updates in the backward, ``step_elements`` and the sharded updates;
``update="allreduce"`` is the plan. It composes with schedules, the guard, accumulation, the
weight EMA, ``no_decay``, soft targets and every gradient-sync strategy. ``state_dict`` has
torch.optim.SGD's layout (``momentum_buffer``) plus ``ortho`` (parameter indices), ``ns_steps``
and ``nesterov`` in the group. On the CPU ``_cpu_step`` is the rule above on fp32 tensors with
``torch.matmul`` in fp32 on the bf16-rounded operands: the oracle of the kernels and the
optimizer of the Gloo paths (there the gradients are multiplied by ``gs`` in place first, for
every tensor).
"""
import numpy as np
import torch

from .sgd import FusedSGD, fma32

NS_COEFFS = (3.4445, -4.7750, 2.0315)
TILE = 32          # muon.hip kMuTile: tile edge, k-step and padding granularity
ITEM_MUON = 0x200  # bit 9 of a work item's kind word (optim.hip kItemMuon)

TENSOR_DTYPE = np.dtype([("p_offset", "<i8"), ("x", "<u8"), ("pitch", "<i4"), ("rest", "<i4"),
                         ("transposed", "<i4"), ("scale", "<f4")])          # api.h MuonTensor
GEMM_DTYPE = np.dtype([("a", "<u8"), ("b", "<u8"), ("e", "<u8"), ("d", "<u8"), ("lda", "<i4"),
                       ("ldb", "<i4"), ("ldd", "<i4"), ("ksteps", "<i4"), ("alpha", "<f4"),
                       ("beta", "<f4"), ("norm0", "<i4"), ("norm_n", "<i4"), ("alpha_pow", "<i4"),
                       ("beta_pow", "<i4"), ("rows", "<i4"), ("cols", "<i4")])  # api.h MuonGemm


def _f32(x):
    return float(np.float32(x))


def _pad(n):
    return -(-int(n) // TILE) * TILE


def device_table(rows, dtype, device):
    """A list of dicts as a device table of ``dtype`` rows (uint8 tensor; missing fields 0)."""
    arr = np.zeros(max(len(rows), 1), dtype=dtype)
    for i, r in enumerate(rows):
        for k, v in r.items():
            arr[i][k] = v
    return torch.from_numpy(arr.view(np.uint8).copy()).to(device)


def tile_items(desc, rows, cols, symmetric):
    """Tile items {desc row, tile row, tile column, mirror} of one padded ``rows x cols`` output;
    ``symmetric``: tiles on or above the diagonal only, the off-diagonal ones mirrored."""
    return [[desc, i, j, int(symmetric)] for i in range(rows // TILE)
            for j in range(i if symmetric else 0, cols // TILE)]


def bf16_round(x):
    return x.to(torch.bfloat16).to(torch.float32)


def newton_schulz(d, ns_steps=5, matmul=torch.matmul, keep=bf16_round):
    """O of the module docstring for one fp32 matrix ``d`` (wide, or it is transposed here and
    back): ``matmul`` multiplies the stored operands (fp32 by default; the tests pass an fp64
    one), ``keep`` is the rounding of every stored matrix. The sum of squares is taken in fp64
    and rounded once to fp32 (the oracle of the kernels' fp32 sums)."""
    if d.shape[0] > d.shape[1]:
        return newton_schulz(d.t().contiguous(), ns_steps, matmul, keep).t().contiguous()
    a, b, c = (torch.tensor(v, dtype=torch.float32) for v in NS_COEFFS)
    S = d.double().pow(2).sum().float()
    s0 = 1.0 / (S.sqrt() + torch.tensor(1e-7, dtype=torch.float32))
    X = keep(d.float())
    for k in range(int(ns_steps)):
        al2, al1, be = (s0 * s0, s0, a * s0) if k == 0 else (None, None, a)
        XXt = matmul(X, X.t()).float()
        A = keep(XXt * al2 if k == 0 else XXt)
        B = keep(fma32(b, A, c * matmul(A, A).float()))
        BX = matmul(B, X).float()
        X = keep(fma32(be, X, BX * al1 if k == 0 else BX))
    return X


class Muon(FusedSGD):
    _rule_launch_only = "Muon's update rule exists in the step's own update launch only"
    metrics_name = "muon"  # the ``optimizer`` field of --metrics records
    needs_whole_tensors = True

    def __init__(self, params, lr=0.02, momentum=0.95, nesterov=True, weight_decay=0.0,
                 ns_steps=5, ortho="conv", grad_scale=1.0, max_grad_norm=None, clip_eps=1e-6,
                 skip_nonfinite=False, no_decay=None):
        if int(ns_steps) < 1:
            raise ValueError("ns_steps must be >= 1")
        super().__init__(params, lr=lr, momentum=momentum, weight_decay=weight_decay,
                         nesterov=False, grad_scale=grad_scale, max_grad_norm=max_grad_norm,
                         clip_eps=clip_eps, skip_nonfinite=skip_nonfinite, no_decay=no_decay)
        if len(self.param_groups) != 1:
            raise ValueError("Muon supports a single param group")
        g = self.param_groups[0]
        g["nesterov"] = self.defaults["nesterov"] = bool(nesterov)  # (also with momentum 0)
        g["ns_steps"] = self.defaults["ns_steps"] = int(ns_steps)
        self._set_ortho(ortho)

    # ----------------------------------------------------------------------------- the tensors
    def _set_ortho(self, spec):
        """``"conv"`` (every 4-D parameter), an iterable of this optimizer's parameters, or — what
        a state dict carries — a list of parameter indices. GPU: allocates the staging buffers
        and the tables, once per distinct set."""
        params = self.param_groups[0]["params"]
        if isinstance(spec, str):
            if spec != "conv":
                raise ValueError(f"ortho = {spec!r}: \"conv\" or an iterable of parameters")
            idx = [i for i, p in enumerate(params) if p.dim() == 4]
        else:
            where = {id(p): i for i, p in enumerate(params)}
            idx = []
            for t in spec:
                if torch.is_tensor(t) and id(t) in where:
                    idx.append(where[id(t)])
                elif isinstance(t, int) and not isinstance(t, bool) and 0 <= t < len(params):
                    idx.append(t)
                else:
                    raise ValueError(f"ortho: {t!r} is neither a parameter of this optimizer nor "
                                     "a parameter index")
        idx = sorted(set(idx))
        for i in idx:
            if params[i].dim() < 2:
                raise ValueError(f"ortho: parameter {i} is not a matrix")
        self.param_groups[0]["ortho"] = idx
        self.defaults["ortho"] = []  # (a group added later orthogonalises nothing)
        self._ortho_row = {i: n for n, i in enumerate(idx)}
        # the staging buffers and every table depend on exactly the set and the iteration count
        key = (tuple(idx), int(self.param_groups[0]["ns_steps"]))
        if self._fused and key != getattr(self, "_staging_key", None):
            self._alloc_staging()
            self._staging_key = key

    def _geometry(self, i):
        """(K, rest, transposed, padded rows, padded columns, scale) of parameter i."""
        p = self.param_groups[0]["params"][i]
        K, rest = p.shape[0], p.numel() // p.shape[0]
        t = K > rest
        m, n = (rest, K) if t else (K, rest)
        return K, rest, t, _pad(m), _pad(n), _f32(np.sqrt(max(1.0, K / rest)))

    def _alloc_staging(self):
        """Two X matrices, A and B per orthogonalised tensor in one zeroed bf16 buffer, and the
        tables whose rows hold their addresses: the stage's and the update's MuonTensor rows and
        3 * ns_steps slices of MuonGemm rows. Nothing here is written on the host again."""
        a, dev = self.arena, self.arena.data.device
        ns = int(self.param_groups[0]["ns_steps"])
        idx = self.param_groups[0]["ortho"]
        geo = [self._geometry(i) for i in idx]
        sizes = [2 * mp * np_ + 2 * mp * mp for _, _, _, mp, np_, _ in geo]
        starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._staging = torch.zeros(max(int(starts[-1]), 1), dtype=torch.bfloat16, device=dev)
        self._muon_partial = torch.zeros(max(self._n_chunks, 1), dtype=torch.float32, device=dev)
        base = self._staging.data_ptr()
        ca, cb, cc = (_f32(v) for v in NS_COEFFS)
        stage, out, gemm = [], [], [[] for _ in range(3 * ns)]
        self._mm_items, self._mn_items = [], []  # per tensor
        for n, (i, (K, rest, t, mp, np_, scale)) in enumerate(zip(idx, geo)):
            x = [base + 2 * int(starts[n]), base + 2 * int(starts[n] + mp * np_)]
            A = base + 2 * int(starts[n] + 2 * mp * np_)
            B = A + 2 * mp * mp
            m, nn = (rest, K) if t else (K, rest)
            row = {"p_offset": a.offsets[i], "pitch": np_, "rest": rest, "transposed": int(t),
                   "scale": scale}
            stage.append(dict(row, x=x[0]))
            out.append(dict(row, x=x[ns % 2]))
            norm = {"norm0": self._chunk0[i], "norm_n": -(-a.numels[i] // self.CHUNK)}
            for k in range(ns):
                cur, nxt = x[k % 2], x[(k + 1) % 2]
                first = k == 0
                gemm[3 * k].append(dict(
                    a=cur, b=cur, e=0, d=A, lda=np_, ldb=np_, ldd=mp, ksteps=np_ // TILE,
                    alpha=1.0, beta=0.0, rows=m, cols=m,
                    **(dict(norm, alpha_pow=2) if first else {})))
                gemm[3 * k + 1].append(dict(
                    a=A, b=A, e=A, d=B, lda=mp, ldb=mp, ldd=mp, ksteps=mp // TILE, alpha=cc,
                    beta=cb, rows=m, cols=m))
                gemm[3 * k + 2].append(dict(
                    a=B, b=cur, e=cur, d=nxt, lda=mp, ldb=np_, ldd=np_, ksteps=mp // TILE,
                    alpha=1.0, beta=ca, rows=m, cols=nn,
                    **(dict(norm, alpha_pow=1, beta_pow=1) if first else {})))
            self._mm_items.append(tile_items(n, mp, mp, True))
            self._mn_items.append(tile_items(n, mp, np_, False))
        self._stage_rows = device_table(stage, TENSOR_DTYPE, dev)
        self._out_rows = device_table(out, TENSOR_DTYPE, dev)
        self._gemm_rows = [device_table(r, GEMM_DTYPE, dev) for r in gemm]
        self._range_tables = {}
        self._muon_tables, self._muon_for = {}, None

    def _range(self, rng):
        """Per parameter range: the stage's chunk items (fourth field: the tensor's table row)
        and the two tile-item tables of its orthogonalised tensors."""
        t = self._range_tables.get(rng)
        if t is None:
            a, dev = self.arena, self.arena.data.device
            rows = [n for i, n in self._ortho_row.items() if rng[0] <= i < rng[1]]
            chunks = [[a.offsets[i] + s0, min(self.CHUNK, a.numels[i] - s0), self._chunk0[i] + c, n]
                      for i, n in self._ortho_row.items() if rng[0] <= i < rng[1]
                      for c, s0 in enumerate(range(0, a.numels[i], self.CHUNK))]
            mm = [it for n in rows for it in self._mm_items[n]]
            mn = [it for n in rows for it in self._mn_items[n]]
            dt = lambda r: torch.tensor(r, dtype=torch.int32, device=dev) if r else None  # noqa: E731
            t = (dt(chunks), len(chunks), dt(mm), len(mm), dt(mn), len(mn))
            self._range_tables[rng] = t
        return t

    def _muon_table(self, key, items):
        """The work-item table ``key`` of FusedSGD._work_table with bit 9 on the items of the
        orthogonalised tensors, and the side table of their MuonTensor rows."""
        if self._muon_for is not self._tables:  # the work tables were rebuilt
            self._muon_tables, self._muon_for = {}, self._tables
        t = self._muon_tables.get(key)
        if t is None:
            side = [self._ortho_row.get(i, -1) for i in self._tables[key][2]]
            s = torch.tensor(side, dtype=torch.int32, device=items.device)
            marked = items.clone()
            marked[:, 0] |= (s >= 0).to(torch.int32) * ITEM_MUON
            t = (marked, s)
            self._muon_tables[key] = t
        return t

    # ---------------------------------------------------------------------------------- step
    @torch.no_grad()
    def _cpu_step(self, params=None):
        """The module docstring's rule for the orthogonalised tensors, torch's own functional
        ``sgd`` for the others (bitwise FusedSGD's CPU step); the gradients are already scaled."""
        from torch.optim.sgd import sgd
        g = self.param_groups[0]
        lr, mu = np.float32(self._cpu_lr()), _f32(g["momentum"])
        plist = g["params"]
        rng = range(*(params if params is not None else (0, len(plist))))
        for masked in (False, True):
            ps = [plist[i] for i in rng if i not in self._ortho_row
                  and plist[i].grad is not None and (i in self._no_decay) == masked]
            if not ps:
                continue
            bufs = [self.state[p].get("momentum_buffer") for p in ps]
            sgd(ps, [p.grad for p in ps], bufs, weight_decay=0.0 if masked else g["weight_decay"],
                momentum=g["momentum"], lr=float(g["lr"]), dampening=0.0, nesterov=g["nesterov"]
                and g["momentum"] != 0, maximize=False, has_sparse_grad=False, foreach=False,
                fused=False, grad_scale=None, found_inf=None)
            if g["momentum"] != 0:
                for p, b in zip(ps, bufs):
                    self.state[p]["momentum_buffer"] = b
        for i in rng:
            p = plist[i]
            if i not in self._ortho_row or p.grad is None:
                continue
            st = self.state[p]
            if st.get("momentum_buffer") is None:
                st["momentum_buffer"] = torch.zeros_like(p, dtype=torch.float32)
            m = st["momentum_buffer"]
            G = p.grad.float()
            m.copy_(fma32(mu, m, G))
            d = fma32(mu, m, G) if g["nesterov"] else m
            K = p.shape[0]
            O = newton_schulz(d.reshape(K, -1).contiguous(), g["ns_steps"]).reshape(p.shape)
            self.apply_ortho(i, O, lr)

    @torch.no_grad()
    def apply_ortho(self, i, O, lr):
        """The rule's last line for parameter i with a given O (the tests hand in the device's)."""
        p = self.param_groups[0]["params"][i]
        nls = float(-(np.float32(lr) * np.float32(self._geometry(i)[5])))
        nlw = float(-(np.float32(lr) * np.float32(self._wd_of(i))))
        pf = p.detach().float()
        p.copy_(fma32(nls, O.float(), fma32(nlw, pf, pf)))

    @torch.no_grad()
    def step(self, closure=None, zero_grad=False, counter=None, skip=None, params=None,
             stream=None, fused_taken=False, signal=None, lr_advance=None, norm_done=False):
        """FusedSGD.step with the Muon rule (same arguments, same captured behaviour): the stage
        launch and 3 * ns_steps grouped GEMM launches over the orthogonalised tensors of the
        range in front of the update launch."""
        if fused_taken:
            raise RuntimeError(self.launch_only_reason + ": no update is taken in the backward "
                               "(fused_taken)")
        if lr_advance is None:
            lr_advance = params is None
        if not self._fused:
            out = None
            if closure is not None:
                with torch.enable_grad():
                    out = closure()
            c, skipped = self._cpu_guard(lr_advance) if self.guarded else \
                (torch.ones((), dtype=torch.float32), False)
            if skipped:
                self._cpu_lr()
            else:
                self._cpu_scale_grads(c)
                self._cpu_step(params)
                self._cpu_ema(params)
            if lr_advance:
                self.count_step()
            if zero_grad:
                self.zero_grad()
            return out
        from ..ops.common import native, stream_handle
        s = stream.cuda_stream if stream is not None else stream_handle()
        a, g = self.arena, self.param_groups[0]
        rng = tuple(params) if params is not None else (0, len(a.params))
        items, n_items, descs = self._work_table(params)
        marked, side = self._muon_table((rng, frozenset(), frozenset()), items)
        chunks, n_chunks, mm, n_mm, mn, n_mn = self._range(rng)
        if self.guarded and not norm_done:
            self.grad_sumsq(params, stream)
        nat = native()
        if n_chunks:
            clip = {k: v for k, v in self._clip_kw(False).items() if k != "clip_stats"}
            nat.muon_stage(chunks.data_ptr(), n_chunks, self._stage_rows.data_ptr(),
                           a.grad.data_ptr(), self.momentum_buffer.data_ptr(),
                           float(g["momentum"]), float(self._grad_scale_factor),
                           int(bool(g["nesterov"])), self._muon_partial.data_ptr(), s, **clip)
            part = self._muon_partial.data_ptr()
            for k in range(int(g["ns_steps"])):
                rows = self._gemm_rows[3 * k:3 * k + 3]
                nat.muon_gemm(mm.data_ptr(), n_mm, rows[0].data_ptr(), part, 0, s)
                nat.muon_gemm(mm.data_ptr(), n_mm, rows[1].data_ptr(), part, 1, s)
                nat.muon_gemm(mn.data_ptr(), n_mn, rows[2].data_ptr(), part, 1, s)
        self._update_launch(marked, n_items, s, descs=descs, zero_grad=zero_grad, counter=counter,
                            skip=skip, signal=signal, lr_advance=lr_advance,
                            muon_side=side.data_ptr(), muon_tensors=self._out_rows.data_ptr())
        return None

    def ortho_output(self, i):
        """O of parameter i as the last step's GEMMs left it (GPU), fp32 in the parameter's
        logical shape: for tests and diagnostics."""
        K, rest, t, mp, np_, _ = self._geometry(i)
        n = self._ortho_row[i]
        row = np.frombuffer(self._out_rows.cpu().numpy().tobytes(), dtype=TENSOR_DTYPE)[n]
        off = (int(row["x"]) - self._staging.data_ptr()) // 2
        X = self._staging[off:off + mp * np_].view(mp, np_).float()
        flat = (X[:rest, :K].t() if t else X[:K, :rest]).reshape(-1)  # [K][rest], arena columns
        shape = self.arena.params[i].shape
        if self.arena.krsc[i]:
            K4, C, R, S = shape
            return flat.view(K4, R, S, C).permute(0, 3, 1, 2).contiguous()
        return flat.view(shape).contiguous()

    # ----------------------------------------------------------------------------- checkpoints
    def load_state_dict(self, sd):
        saved = sd["param_groups"][0] if sd.get("param_groups") else {}
        g = self.param_groups[0]
        keep = {k: saved.get(k, g[k]) for k in ("ortho", "ns_steps", "nesterov")}
        out = super().load_state_dict(sd)
        g = self.param_groups[0]
        g["ns_steps"], g["nesterov"] = int(keep["ns_steps"]), bool(keep["nesterov"])
        self._set_ortho([int(i) for i in keep["ortho"]])
        return out

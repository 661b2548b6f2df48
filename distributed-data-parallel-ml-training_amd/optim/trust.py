"""The tables of a per-tensor trust ratio inside the fused update launch, shared by LARS
(optim/lars.py) and LAMB (optim/lamb.py): which tensors are adapted, the per-parameter table
{first global chunk, chunks, adapted, -}, the chunk items of the norms launch and the side table
parallel to the update launch's work items (csrc/kernels/api.h LarsArgs / LambArgs). A mixin in
front of FusedSGD: it reads ``param_groups[0]["exclude_1d"]``, the arena and FusedSGD's tables.
"""
import torch


class TrustTables:
    needs_whole_tensors = True

    def _alloc_trust_tables(self):
        """The partial sums ({.., ..} per global chunk), the ratios and the tensor table on the
        GPU: allocated once, so captured launches keep these addresses."""
        self._trust_cpu = None
        if self._fused:
            a, dev = self.arena, self.arena.data.device
            self._trust_partial = torch.zeros(max(self._n_chunks, 1), 2, dtype=torch.float32,
                                              device=dev)
            self._trust_dev = torch.ones(len(a.params), dtype=torch.float32, device=dev)
            self._trust_tensors = torch.zeros(len(a.params), 4, dtype=torch.int32, device=dev)
            self._adapted_for = None
            self._norm_tables = {}
            self._side_tables, self._side_for = {}, None

    def _adapted(self):
        ex = bool(self.param_groups[0]["exclude_1d"])
        return [p.dim() > 1 or not ex for p in self.param_groups[0]["params"]]

    def _tensor_table(self):
        """Per parameter {first global chunk, chunks, adapted, -}: written in place when
        ``exclude_1d`` changes (not inside a capture: change it before capturing)."""
        ex = bool(self.param_groups[0]["exclude_1d"])
        if self._adapted_for != ex:
            ad, a = self._adapted(), self.arena
            rows = [[self._chunk0[i], -(-a.numels[i] // self.CHUNK), int(ad[i]), 0]
                    for i in range(len(a.params))]
            self._trust_tensors.copy_(torch.tensor(rows, dtype=torch.int32))
            self._adapted_for = ex
            self._norm_tables = {}
        return self._trust_tensors

    def _norm_table(self, rng):
        """Work items of the norms launch over parameters [i0, i1): FusedSGD._chunk_table over
        the adapted tensors; cached per range."""
        if rng not in self._norm_tables:
            self._norm_tables[rng] = self._chunk_table(rng, self._adapted())
        return self._norm_tables[rng]

    def _side_table(self, key):
        """Side table parallel to the work-item table ``key`` of FusedSGD._work_table: per item
        {parameter index | -1, 1 on the tensor's first item (that block stores the ratio)}."""
        if self._side_for is not self._tables:  # the work tables were rebuilt
            self._side_tables, self._side_for = {}, self._tables
        t = self._side_tables.get(key)
        if t is None:
            seen, rows = set(), []
            for i in self._tables[key][2]:
                rows.append([i, int(i >= 0 and i not in seen)])
                seen.add(i)
            t = torch.tensor(rows, dtype=torch.int32, device=self.arena.data.device)
            self._side_tables[key] = t
        return t

    def _trust_kw(self, prefix, rng):
        """The four table keywords of the native update launch over parameters ``rng`` (call
        after ``_work_table`` of the same range)."""
        side = self._side_table((rng, frozenset(), frozenset()))
        return {f"{prefix}_side": side.data_ptr(),
                f"{prefix}_tensors": self._tensor_table().data_ptr(),
                f"{prefix}_partial": self._trust_partial.data_ptr(),
                f"{prefix}_trust": self._trust_dev.data_ptr()}

    def trust_ratios(self):
        """Per-parameter trust ratios of the last update of each tensor (1.0: not adapted, or a
        zero norm). GPU: the device array the update kernel writes, as is (no sync)."""
        if self._fused:
            return self._trust_dev
        if self._trust_cpu is None:
            self._trust_cpu = torch.ones(len(self.param_groups[0]["params"]))
        return self._trust_cpu

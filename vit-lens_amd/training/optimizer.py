"""`LARS`, the optimizer of the reference's linear probe (training/optimizer.py; layer-wise adaptive rate scaling in the
MoCo v3 form: no rate scaling and no weight decay for tensors of at most one dimension).  A torch.optim.Optimizer with the
reference's constructor, param_groups and per-parameter state key "mu", so schedulers, state_dict() and resume behave as
there; step() is ONE vl_lars_multi_step call per parameter group - the two norms of every tensor and the trust ratio stay on
the device."""
import torch


class LARS(torch.optim.Optimizer):
    def __init__(self, params, lr=0, weight_decay=0, momentum=0.9, trust_coefficient=0.001):
        defaults = dict(lr=lr, weight_decay=weight_decay, momentum=momentum, trust_coefficient=trust_coefficient)
        super().__init__(params, defaults)
        self._tables = {}          # group index -> (key, device slot table, workspace)

    @torch.no_grad()
    def step(self):
        from vitlens_hip import ops
        for gi, group in enumerate(self.param_groups):
            rows = []
            for p in group["params"]:
                if p.grad is None:
                    continue
                state = self.state[p]
                if "mu" not in state:
                    state["mu"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                rows.append((p.data, g, state["mu"], group["weight_decay"], p.ndim > 1))
            if not rows:
                continue
            key = tuple((r[0].data_ptr(), r[1].data_ptr(), r[2].data_ptr(), r[0].numel(), float(r[3]), r[4]) for r in rows)
            cached = self._tables.get(gi)
            if cached is None or cached[0] != key:          # packed once; again only when a tensor moved (a new .grad, .to())
                dev = rows[0][0].device
                slots = ops.pack_lars_slots(rows).to(dev)
                total = sum(r[0].numel() for r in rows)
                ws = torch.empty(ops.lars_ws_floats(total, len(rows)) // 2 + 1, device=dev, dtype=torch.float64)
                cached = self._tables[gi] = (key, slots, ws)
            for at in range(0, len(rows), ops.LARS_MAX_SLOTS):
                n = min(ops.LARS_MAX_SLOTS, len(rows) - at)
                ops.lars_multi_step(cached[1][at:at + n], n, group["lr"], group["momentum"], group["trust_coefficient"], ws=cached[2])

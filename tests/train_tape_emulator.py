"""Float64 emulator of the TRAIN tapes (``engine.compile_net(..., train=True)``) — TEST INFRASTRUCTURE.

``tests/tape_emulator.py`` with the two op kinds of MAP training, following their definitions in ``include/lip.h``
literally, and the three engine calls of a training step around them (train primal, refresh of the transposed kernels,
train backward).
"""
import torch

from lip_amd import _native as nv
from lip_amd.engine import BN_MOMENTUM
from tape_emulator import F64, TapeMachine


class TrainTapeMachine(TapeMachine):
    def __init__(self, cn, theta, consts, Z):
        super().__init__(cn, theta, consts, Z, 1)
        self.consts = self.consts.clone()
        self.work = torch.zeros(max(cn.work_pp, cn.train_work_pp), dtype=F64)
        # op.bn_eps and op.fscale are C floats: the exact eps of the unit, found by its running-mean slot
        self.unit_at = {item[2]: item[1] for item in cn.const_plan if item[0] == "run"}

    def bn_stats(self, op):
        R, N = op.n_img * op.OH * op.OW, op.N
        y = self.view(op.seg[0].a, 1, R * N).reshape(R, N)
        if op.e0.space != nv.SP_NONE:
            y = y + self.view(op.e0, 1, N)
        mean = y.sum(0) / R
        var = ((y - mean) ** 2).sum(0) / R
        u = self.unit_at[op.out.off]
        assert abs(op.bn_eps - u.bn_eps) <= 1e-7 * u.bn_eps and abs(op.fscale - BN_MOMENTUM) < 1e-7
        rstd = 1.0 / torch.sqrt(var + u.bn_eps)
        self.view(op.aux0, 1, N).copy_(mean.reshape(1, N))
        self.view(op.aux1, 1, N).copy_(rstd.reshape(1, N))
        self.view(op.scale, 1, N).copy_((self.view(op.e1, 1, N).reshape(N) * rstd).reshape(1, N))
        mom = BN_MOMENTUM
        rm, rv = self.view(op.out, 1, N), self.view(op.out2, 1, N)
        rm.copy_(mom * rm + (1 - mom) * mean.reshape(1, N))
        rv.copy_(mom * rv + (1 - mom) * var.reshape(1, N))

    def bn_train_bwd(self, op, P):
        R, N = op.n_img * op.OH * op.OW, op.N
        g = self.view(op.seg[0].a, P, R * N).reshape(P, R, N)
        xh = self.view(op.xhat, 1, R * N).reshape(1, R, N)
        db = self.view(op.e0, P, N).reshape(P, 1, N)
        dg = self.view(op.e1, P, N).reshape(P, 1, N)
        self.view(op.out, P, R * N).copy_((g - (db + xh * dg) / R).reshape(P, R * N))

    def run_op(self, op, P, mode=0, c=1.0):
        if op.kind == nv.OP_BN_STATS:
            self.bn_stats(op)
        elif op.kind == nv.OP_BN_TRAIN_BWD:
            self.bn_train_bwd(op, P)
        else:
            super().run_op(op, P, mode, c)

    # ------------------------------------------------------------------ the calls of a training step
    def train_primal(self):
        for op in self.cn.train_tapes[0]:
            self.run_op(op, 1)

    def refresh(self):
        """Wt[kh][kw][co][ci] = W[kh][kw][ci][co] * s[co] for every 'wt' entry of the constants plan"""
        for item in self.cn.const_plan:
            if item[0] != "wt":
                continue
            _, u, wo, so = item
            koff = self.cn.offsets[u.kernel][0]
            W = self.theta[koff:koff + u.kh * u.kw * u.cin * u.cout].reshape(u.kh * u.kw, u.cin, u.cout)
            if so is not None:
                W = W * self.consts[so:so + u.cout]
            self.consts[wo:wo + W.numel()] = W.permute(0, 2, 1).reshape(-1)

    def train_backward(self, U):
        self.H = U.to(F64).contiguous().reshape(-1)
        self.Y = torch.zeros(self.cn.D, dtype=F64)
        for op in self.cn.train_tapes[1]:
            self.run_op(op, 1, nv.HEAD_IN, 1.0)
        return self.Y

    def logits(self):
        o = self.cn.a_off[self.cn.net.out]
        return self.prim[o:o + self.cn.n * self.cn.K].reshape(self.cn.n, self.cn.K)

    def running_stats(self):
        """{bn_mean path: (K,), bn_var path: (K,)} read back from the constants"""
        out = {}
        for item in self.cn.const_plan:
            if item[0] == "run":
                _, u, mo, vo = item
                out[u.bn_mean] = self.consts[mo:mo + u.cout].clone()
                out[u.bn_var] = self.consts[vo:vo + u.cout].clone()
        return out

"""BiDateNet: drop-in for the reference's models/bidate_model.py:7-40.

Same constructor, same ``forward(x_d1, x_d2)`` (two [B,C,H,W] float32 tensors ->
[B,n_classes,H,W] float32 logits that take part in autograd), same sub-module
tree / ``state_dict()`` schema, ``.train()/.eval()`` switch BatchNorm mode.  The
whole forward + backward runs on the gfx950 HIP library; there is no CPU path.
"""
import os

import torch
import torch.nn as nn

from .unet_parts import down, outconv, up, inconv
from .._lib import FUSIONS
from ..engine import BiDateEngine


class _Lease:
    """Marks an engine workspace as owned by one autograd graph.  Released at the END of that graph's backward() -- not when
    the grad_fn node dies: in the usual loop `logits` / `loss` of the previous iteration are still bound when the next
    forward runs, and a lease held until then would make the loop ping-pong between two full workspaces -- or, without a
    backward, when the graph is freed.  A workspace carries a generation counter: a second backward through the same graph
    (retain_graph=True) after another forward reused the buffers raises instead of reading overwritten activations."""

    def __init__(self, ws):
        self.ws = ws
        ws.leased = True
        self.generation = ws.generation       # engine.forward bumped it when it filled the buffers

    def release(self):
        if self.ws is not None and self.ws.generation == self.generation:
            self.ws.leased = False
        self.ws_released = True

    def __del__(self):
        if not getattr(self, 'ws_released', False):
            self.release()


class _BiDateFunction(torch.autograd.Function):
    """One autograd node for the whole network: forward enqueues the fused HIP schedule, backward the
    hand-written backward schedule (no autograd tape through individual ops).

    Training mode: backward reads the activations the forward left in its (leased) workspace.  Eval mode: the forward is the
    ordinary eval forward; backward RECOMPUTES the training-layout forward on the running statistics the forward saw (copied at
    forward time: a training forward in between moves the buffers in place) and runs the frozen-BatchNorm backward on it.  The
    gradient on an input image is returned only when that input requires grad, a parameter's only when it requires grad (a
    layer whose conv weight does not launches no weight-gradient GEMM)."""

    @staticmethod
    def forward(ctx, module, x_d1, x_d2, *params):
        eng = module.engine()
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            eng.check_input_grad()            # ValueError above 16 bands, here and not from the middle of backward
        P = dict(module.state_dict(keep_vars=True))
        training = module.training
        logits, ws = eng.forward(x_d1.detach(), x_d2.detach(), {k: v.detach() for k, v in P.items()}, training)
        ctx.module, ctx.ws, ctx.training = module, ws, training
        ctx.n_params = len(params)
        if training and any(ctx.needs_input_grad):
            ctx.lease = _Lease(ws)            # nobody else may run a forward on these buffers while this graph lives
        elif any(ctx.needs_input_grad):
            # eval graph: backward recomputes the forward from these (autograd's version check refuses an in-place change of any of them)
            ctx.save_for_backward(x_d1, x_d2, *params)
            ctx.running = torch.cat([P[f'{L.bn}.{b}'].detach() for L in eng.layers for b in ('running_mean', 'running_var')])
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        module = ctx.module
        eng = module.engine()
        named = list(module.named_parameters())
        needs = ctx.needs_input_grad
        P = {k: v.detach() for k, v in module.state_dict(keep_vars=True).items()}
        grads = {k: torch.empty_like(p, dtype=torch.float32) for k, p in named}
        need = {k for i, (k, _) in enumerate(named) if needs[3 + i]}
        dx = None
        if needs[1] or needs[2]:
            x = dlogits
            B, _, H, W = x.shape
            dx = tuple(torch.empty(B, eng.n_channels, H, W, dtype=torch.float32, device=x.device) for _ in range(2))
        if ctx.training:
            lease = getattr(ctx, 'lease', None)
            if lease is not None and ctx.ws.generation != lease.generation:
                raise RuntimeError('fabric_amd: this graph\'s activations were overwritten by a later forward (second backward with '
                                   'retain_graph=True after another forward of the same shape): re-run the forward')
            eng.backward(ctx.ws, dlogits, P, grads, dx=dx, need=need)
            if lease is not None:
                lease.release()               # the activations are dead: the next forward of this shape reuses the workspace
        else:
            x_d1, x_d2 = ctx.saved_tensors[:2]
            off = 0
            for L in eng.layers:              # the running statistics as the forward saw them
                for b in ('running_mean', 'running_var'):
                    P[f'{L.bn}.{b}'] = ctx.running[off:off + L.cout]
                    off += L.cout
            _, ws = eng.forward(x_d1.detach(), x_d2.detach(), P, training=False, frozen=True)
            lease = _Lease(ws)                # a forward of this shape in a hook would otherwise take these buffers
            try:
                eng.backward(ws, dlogits, P, grads, dx=dx, bn_mode='running', need=need)
            finally:
                lease.release()
                if eng.x3:
                    ws.release_split()        # the recompute's per-layer split operands (as model.train(False) drops them)
        dxs = (dx[0] if dx is not None and needs[1] else None, dx[1] if dx is not None and needs[2] else None)
        return (None,) + dxs + tuple(grads[k] if needs[3 + i] else None for i, (k, _) in enumerate(named))


class BiDateNet(nn.Module):
    def __init__(self, n_channels, n_classes, precision=None, fusion='product'):
        super(BiDateNet, self).__init__()
        if fusion not in FUSIONS:
            raise ValueError(f"fusion must be 'product' or 'absdiff', got {fusion!r}")
        self.inc = inconv(n_channels, 64)
        self.down1 = down(64, 128)
        self.down2 = down(128, 256)
        self.down3 = down(256, 512)
        self.down4 = down(512, 512)

        self.up1 = up(1024, 256)
        self.up2 = up(512, 128)
        self.up3 = up(256, 64)
        self.up4 = up(128, 64)
        self.outc = outconv(64, n_classes)

        self.n_channels, self.n_classes = n_channels, n_classes
        # 'bf16' = throughput setting; 'bf16x3' = float32 tensors with split bf16 GEMM operands (logits within 1e-3 of the reference at
        # matrix-core speed); 'fp32' = exact f32 MFMA
        self.precision = precision or os.environ.get('BIDATE_PRECISION', 'bf16')
        # how the two dates' encoder features meet in the skips: 'product' = relu(x_d2 * x_d1), the reference's models/bidate_model.py:35-38;
        # 'absdiff' = |x_d2 - x_d1| (FC-Siam-diff).  No parameters: the state dict is the same.  Read when the engine is built; assigning
        # another value rebuilds the engine at the next call, as `precision` does.
        self.fusion = fusion
        self._engine = None

    def engine(self):
        if self._engine is None or self._engine.precision != self.precision or self._engine.fusion != self.fusion:
            self._engine = BiDateEngine(self.n_channels, self.n_classes, self.precision, self.fusion)     # ValueError for an unknown fusion
        return self._engine

    def forward(self, x_d1, x_d2):
        params = [p for _, p in self.named_parameters()]
        return _BiDateFunction.apply(self, x_d1, x_d2, *params)

    # the packed bf16 / f32 GEMM images are derived from the master weights: anything that rewrites parameters behind
    # autograd's version counters has to drop them
    def load_state_dict(self, *args, **kw):
        out = super().load_state_dict(*args, **kw)
        if getattr(self, '_engine', None) is not None:
            self._engine.invalidate_weights()
        return out

    def _apply(self, fn, *args, **kw):
        out = super()._apply(fn, *args, **kw)
        if getattr(self, '_engine', None) is not None:
            self._engine.invalidate_weights()
        return out

    def train(self, mode=True):
        """nn.Module.train / eval; leaving training mode also drops the bf16x3 setting's per-layer operand-split buffers (about 1.5 GB
        per trained workspace at B=16, 128x128; re-grown on demand by the next training forward)."""
        out = super().train(mode)
        if not mode and getattr(self, '_engine', None) is not None and self._engine.x3:
            self._engine.release_split_buffers()
        return out

    # the engine and its workspaces are derived state: keep them out of pickles / deepcopies
    def __getstate__(self):
        d = self.__dict__.copy()
        d['_engine'] = None
        return d

    def __setstate__(self, state):
        """Unpickling.  The reference persists a model ONLY as a whole-module pickle (train.py:222 `torch.save(model, ...)` of
        nn.DataParallel(BiDateNet(13, 2)), utils/helpers.py:333-335).  Such a pickle resolves its class paths to this class through the
        root `models.*` shims, but its __dict__ is the reference's: sub-modules and parameters only.  Everything this class adds is
        derived state and is rebuilt here: the channel counts from the first / last convolution, the numerics setting from
        BIDATE_PRECISION (default 'bf16'), the date fusion 'product' (the reference's only one), no engine yet."""
        super().__setstate__(state)
        d = self.__dict__
        if 'n_channels' not in d:
            d['n_channels'] = int(self.inc.conv.conv[0].weight.shape[1])
        if 'n_classes' not in d:
            d['n_classes'] = int(self.outc.conv.weight.shape[0])
        if d.get('precision') is None:
            d['precision'] = os.environ.get('BIDATE_PRECISION', 'bf16')
        if d.get('fusion') is None:                # the reference's pickles and pickles of this class from before it had the attribute
            d['fusion'] = 'product'
        d['_engine'] = None

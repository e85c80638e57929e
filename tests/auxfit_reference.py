"""Float64 numpy restatement of include/rcu_fit.h "Auxiliary fit": the train-mode loss of a PostNet on a feature map, its exact gradient, the
batch statistics, the running-statistics update and Adam's step, with the condition sums the GPU tests bound the device's errors with.  Nothing of
the package is imported; the fixture tests/golden/g36_auxfit.npz (tests/golden/generate_auxfit.py) holds what torch's own modules give."""
import numpy as np

EPS = 1e-5
CHUNK = 1024          # RCU_DENSITY_CHUNK: voxels a float32 accumulator covers
U = 2.0 ** -24        # unit roundoff of float32


def packing(F, L):
    """[(state_dict name, shape)] in the order of the flat parameter / gradient array of include/rcu_fit.h."""
    rows = []
    for k in range(L):
        base = 'convs.{}.conv2d_batch_relu.'.format(k)
        rows += [(base + 'conv.weight', (F, F)), (base + 'conv.bias', (F,)), (base + 'bn.weight', (F,)), (base + 'bn.bias', (F,))]
    return rows + [('conv_logits.weight', (2, F)), ('conv_logits.bias', (2,))]


def param_count(F, L):
    return sum(int(np.prod(shape)) for _, shape in packing(F, L))


def pack(params, F, L, dtype=np.float32):
    """dict name -> array (conv weights may be [F, F, 1, 1]) -> the flat array."""
    return np.concatenate([np.asarray(params[name], dtype=np.float64).reshape(shape).ravel() for name, shape in packing(F, L)]).astype(dtype)


def unpack(flat, F, L):
    out, at = {}, 0
    for name, shape in packing(F, L):
        size = int(np.prod(shape))
        out[name] = np.asarray(flat[at:at + size]).reshape(shape)
        at += size
    assert at == len(flat)
    return out


def loss_and_grad(phi, e, params, L):
    """phi float [N, F], e integer [N] in {0, 1}, params: dict name -> array.  -> dict with loss, grads (name -> float64 array), mu, var [L, F], the
    per-voxel tensors du, dy, xhat, a (lists over the layers; a[0] = phi), dz, the per-voxel loss, and cond: name -> the condition sum of every
    gradient entry, sum_v |du_i(v)| |a_j(v)| (bias: a = 1; beta, gamma: sum_v |dy_i|, sum_v |dy_i| |xhat_i|; output layer: dz for du)."""
    phi = np.asarray(phi, dtype=np.float64)
    N, F = phi.shape
    assert N >= 2
    p = {k: np.asarray(v, dtype=np.float64) for k, v in params.items()}
    names = ['convs.{}.conv2d_batch_relu.'.format(k) for k in range(L)]
    a, u, xhat, y, mu, var = [phi], [], [], [], [], []
    for k in range(L):
        W, b = p[names[k] + 'conv.weight'].reshape(F, F), p[names[k] + 'conv.bias']
        uk = a[-1] @ W.T + b
        m = uk.mean(0)
        v = ((uk - m) ** 2).mean(0)
        xk = (uk - m) / np.sqrt(v + EPS)
        yk = p[names[k] + 'bn.weight'] * xk + p[names[k] + 'bn.bias']
        u.append(uk), mu.append(m), var.append(v), xhat.append(xk), y.append(yk), a.append(np.maximum(yk, 0.0))
    Wo, bo = p['conv_logits.weight'].reshape(2, F), p['conv_logits.bias']
    z = a[-1] @ Wo.T + bo
    zmax = z.max(1, keepdims=True)
    lse = zmax[:, 0] + np.log(np.exp(z - zmax).sum(1))
    e = np.asarray(e).astype(np.int64).reshape(N)
    per_voxel = lse - z[np.arange(N), e]
    soft = np.exp(z - lse[:, None])
    dz = soft.copy()
    dz[np.arange(N), e] -= 1.0
    dz /= N
    grads, cond = {}, {}
    grads['conv_logits.weight'], cond['conv_logits.weight'] = dz.T @ a[-1], np.abs(dz).T @ np.abs(a[-1])
    grads['conv_logits.bias'], cond['conv_logits.bias'] = dz.sum(0), np.abs(dz).sum(0)
    da = dz @ Wo
    du, dy = [None] * L, [None] * L
    for k in range(L - 1, -1, -1):
        dyk = np.where(y[k] > 0, da, 0.0)
        gamma = p[names[k] + 'bn.weight']
        duk = gamma / np.sqrt(var[k] + EPS) * (dyk - dyk.mean(0) - xhat[k] * (dyk * xhat[k]).mean(0))
        du[k], dy[k] = duk, dyk
        grads[names[k] + 'conv.weight'], cond[names[k] + 'conv.weight'] = duk.T @ a[k], np.abs(duk).T @ np.abs(a[k])
        grads[names[k] + 'conv.bias'], cond[names[k] + 'conv.bias'] = duk.sum(0), np.abs(duk).sum(0)
        grads[names[k] + 'bn.weight'], cond[names[k] + 'bn.weight'] = (dyk * xhat[k]).sum(0), (np.abs(dyk) * np.abs(xhat[k])).sum(0)
        grads[names[k] + 'bn.bias'], cond[names[k] + 'bn.bias'] = dyk.sum(0), np.abs(dyk).sum(0)
        da = duk @ p[names[k] + 'conv.weight'].reshape(F, F)
    return dict(loss=float(per_voxel.mean()), grads=grads, cond=cond, mu=np.stack(mu), var=np.stack(var), du=du, dy=dy, xhat=xhat, a=a, u=u, dz=dz,
                per_voxel=per_voxel, mean_abs_u=np.stack([np.abs(v).mean(0) for v in u]), mean_abs_loss=float(np.abs(per_voxel).mean()))


def gradient_bound(cond):
    """|g_dev - g64| <= (1024 + 2) 2^-24 A, entry by entry: the float32 accumulation bound of a chunk on the condition sum."""
    return {name: (CHUNK + 2) * U * A for name, A in cond.items()}


def statistics_bounds(ref):
    """(mu bound [L, F], var bound [L, F], loss bound) of the issue: (1024 + 2) u mean|u|;  (1024 + 4) u mean (u - mu)^2 + 2 u var;  (1024 + 2) u mean|l|."""
    return (CHUNK + 2) * U * ref['mean_abs_u'], (CHUNK + 4) * U * ref['var'] + 2 * U * ref['var'], (CHUNK + 2) * U * ref['mean_abs_loss']


def update_running(rm, rv, nbt, mu, var, N, momentum=0.1):
    """torch's BatchNorm2d update of a train-mode forward: the unbiased variance enters the running one."""
    return (1 - momentum) * rm + momentum * mu, (1 - momentum) * rv + momentum * var * N / (N - 1), nbt + 1


def adam_step(params, grads, m, v, t, lr=1e-4, betas=(0.9, 0.999), eps=1e-8):
    """One step of torch.optim.Adam (no weight decay, no amsgrad) on dicts of float64 arrays; t is the 1-based step.  -> (params, m, v)."""
    b1, b2 = betas
    out_p, out_m, out_v = {}, {}, {}
    for name in params:
        g = np.asarray(grads[name], dtype=np.float64).reshape(np.shape(params[name]))
        out_m[name] = b1 * m[name] + (1 - b1) * g
        out_v[name] = b2 * v[name] + (1 - b2) * g * g
        step = lr / (1 - b1 ** t)
        out_p[name] = params[name] - step * out_m[name] / (np.sqrt(out_v[name]) / np.sqrt(1 - b2 ** t) + eps)
    return out_p, out_m, out_v


def fit_steps(phi, e, state, L, steps, lr=1e-4):
    """``steps`` Adam steps on one batch from a float64 state_dict (parameters, running statistics, num_batches_tracked).  -> (state, losses)."""
    F = np.asarray(phi).shape[1]
    state = {k: np.array(v, dtype=np.float64 if np.asarray(v).dtype.kind == 'f' else np.int64) for k, v in state.items()}
    names = [name for name, _ in packing(F, L)]
    params = {name: state[name] for name in names}
    m = {name: np.zeros_like(params[name]) for name in names}
    v = {name: np.zeros_like(params[name]) for name in names}
    losses = []
    N = np.asarray(phi).shape[0]
    for t in range(1, steps + 1):
        ref = loss_and_grad(phi, e, params, L)
        losses.append(ref['loss'])
        for k in range(L):
            bn = 'convs.{}.conv2d_batch_relu.bn.'.format(k)
            state[bn + 'running_mean'], state[bn + 'running_var'], state[bn + 'num_batches_tracked'] = update_running(
                state[bn + 'running_mean'], state[bn + 'running_var'], state[bn + 'num_batches_tracked'], ref['mu'][k], ref['var'][k], N)
        params, m, v = adam_step(params, ref['grads'], m, v, t, lr=lr)
    state.update(params)
    return state, losses

"""The planner alone, without a device: rcu_unet_plan on a shape, a batch size and plan options, read back row by row through rcu_unet_layer_info.
Shared by the planner tests (test_abi_cpu.py, test_fold10_cpu.py, test_upconv4_cpu.py, test_parity_power_cpu.py, test_gpu_deep_levels.py,
test_plan_table_cpu.py) and by tests/golden/generate_plan_table.py."""
import ctypes

DESC_DEFAULTS = dict(nb_classes=2, in_channels=4, depth=4, start_filters=32, has_dropout=1, dropout_center=-1, sigma_out=0, bn=1, residual=0,
                     provide_features=0)


def plan_rows(height, width, max_batch, options=None, **desc):
    """One dict per layer of the plan of a height x width net for max_batch samples.  `desc`: rcu_unet_desc fields other than the shipped BraTS
    architecture's (DESC_DEFAULTS); `options`: rcu_unet_options fields other than rcu_unet_default_options'.  A plan can be inspected, never run."""
    from rcu_amd import _lib
    lib = _lib.load()
    fields = dict(DESC_DEFAULTS, **desc)
    d = _lib.UnetDesc(height=height, width=width, max_batch=max_batch, **{k: int(v) for k, v in fields.items()})
    opts = _lib.UnetOptions()
    lib.rcu_unet_default_options(ctypes.byref(opts))
    for key, value in (options or {}).items():
        assert hasattr(opts, key), key
        setattr(opts, key, value)
    handle = ctypes.c_void_p()
    _lib.check(lib.rcu_unet_plan(ctypes.byref(d), ctypes.byref(opts), ctypes.byref(handle)))
    try:
        assert lib.rcu_unet_finalize_weights(handle) == -4      # RCU_ERR_STATE
        rows = []
        for i in range(lib.rcu_unet_num_layers(handle)):
            info = _lib.LayerInfo()
            _lib.check(lib.rcu_unet_layer_info(handle, i, ctypes.byref(info)))
            rows.append(dict(name=info.name.decode(), kernel=info.kernel.decode(), cin=info.cin, cout=info.cout, height=info.height, width=info.width,
                             grid=(info.grid_height, info.grid_width), upsample=info.upsample, pooled=info.pooled, dual_source=info.dual_source,
                             head_fusable=info.head_fusable, flops=info.flops_per_slice, mfma_flops=info.mfma_flops_per_slice))
        return rows
    finally:
        lib.rcu_unet_destroy(handle)

"""ctypes binding of libdasr_hip.so (include/dasr_hip.h).  Fails loudly when the library is missing:
there is no CPU / PyTorch fallback on the product path."""
import ctypes as C
import os
import struct

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, 'libdasr_hip.so')

c_i32, c_i64, c_f32, c_vp = C.c_int32, C.c_int64, C.c_float, C.c_void_p


class Tensor(C.Structure):
    _fields_ = [('p', c_vp), ('n_stride', c_i64), ('cb_stride', c_i64)]


class ConvParams(C.Structure):
    _fields_ = [('inp', Tensor), ('in_f32', c_i32), ('Hin', c_i32), ('Win', c_i32), ('ups', c_i32), ('cin', c_i32),
                ('w', c_vp), ('w_lo_off', c_i64), ('bias', c_vp),
                ('cout', c_i32), ('Hout', c_i32), ('Wout', c_i32), ('N', c_i32),
                ('kh', c_i32), ('stride', c_i32), ('pad', c_i32), ('prec', c_i32), ('mt', c_i32),
                ('act', c_i32), ('slope', c_f32),
                ('mask', Tensor), ('mask_f32', c_i32),
                ('alpha', c_f32), ('res1', Tensor), ('beta1', c_f32), ('res2', Tensor), ('beta2', c_f32),
                ('out_f32', Tensor), ('out_bf16', Tensor), ('gamma', c_f32), ('xcd_remap', c_i32),
                ('pad_x', c_i32), ('out_stride', c_i32), ('out_oy', c_i32), ('out_ox', c_i32), ('out_W', c_i32), ('slope_ptr', c_vp),
                ('in_stride', c_i32), ('in_oy', c_i32), ('in_ox', c_i32), ('in_W', c_i32), ('in_scale', c_f32), ('out16_f16', c_i32), ('in_wrap', c_i32), ('out16_lo', c_i32), ('res1_lo', c_i32), ('prelu_part', c_vp)]


class WgradPart(C.Structure):
    _fields_ = [('g', Tensor), ('g_f32', c_i32), ('inp', Tensor), ('in_f32', c_i32), ('ups', c_i32), ('n_ctiles', c_i32),
                ('g_planes', c_i32), ('in_planes', c_i32),
                ('Hin', c_i32), ('Win', c_i32), ('Hout', c_i32), ('Wout', c_i32), ('N', c_i32),
                ('kh', c_i32), ('stride', c_i32), ('pad', c_i32), ('want_bias', c_i32),
                ('ws_off', c_i64), ('ws_bias_off', c_i64), ('tap0', c_i32), ('g_scale', c_f32)]


class WgradReducePart(C.Structure):
    _fields_ = [('ws_off', c_i64), ('ws_bias_off', c_i64), ('nsplit', c_i32), ('ntaps', c_i32), ('oc0', c_i32), ('c0', c_i32),
                ('cout', c_i32), ('cin', c_i32), ('n_ctiles', c_i32), ('dst_w_off', c_i64), ('dst_b_off', c_i64),
                ('flip_io', c_i32), ('split_stride', c_i64), ('tap_stride', c_i64), ('bias_stride', c_i64),
                ('tap0', c_i32), ('ntaps_total', c_i32), ('bias_nsplit', c_i32), ('reserved_', c_i32)]


class ResblockParams(C.Structure):
    _fields_ = [('x16', Tensor), ('x32', Tensor), ('w0', c_vp), ('b0', c_vp), ('w1', c_vp), ('b1', c_vp),
                ('y32', Tensor), ('y16', Tensor), ('h', Tensor), ('N', c_i32), ('H', c_i32), ('W', c_i32), ('res_scale', c_f32), ('slope', c_f32)]


class PackSeg(C.Structure):
    _fields_ = [('src_off', c_i64), ('src_cout', c_i32), ('src_cin', c_i32), ('cin_start', c_i32), ('cin_len', c_i32),
                ('src_c0', c_i32), ('transpose', c_i32)]


class PackDesc(C.Structure):
    _fields_ = [('dst_off', c_i64), ('lo_off', c_i64), ('cout', c_i32), ('cin_pad', c_i32), ('ntaps', c_i32), ('mt', c_i32),
                ('nseg', c_i32), ('src_ntaps', c_i32), ('fmt', c_i32), ('tapmap', C.c_int8 * 32), ('tapmask', C.c_uint16 * 16), ('seg', PackSeg * 5)]


class CropDesc(C.Structure):
    _fields_ = [('src', c_vp), ('C', c_i32), ('H', c_i32), ('W', c_i32), ('vH', c_i32), ('vW', c_i32), ('y0', c_i32), ('x0', c_i32), ('flags', c_i32)]


class CropU8Desc(C.Structure):
    """dasr_crop_u8_desc"""
    _fields_ = [('src', c_vp), ('H', c_i32), ('W', c_i32), ('y0', c_i32), ('x0', c_i32), ('crop', c_i32), ('flags', c_i32), ('sub_y', c_i32), ('sub_x', c_i32)]


class SrnU8Desc(C.Structure):
    """dasr_srn_u8_desc"""
    _fields_ = [('src', c_vp), ('H', c_i32), ('W', c_i32), ('y0', c_i32), ('x0', c_i32), ('size', c_i32), ('flags', c_i32), ('dst', c_vp)]


class WindowDesc(C.Structure):
    """dasr_window_desc"""
    _fields_ = [('y0', c_i32), ('x0', c_i32)]


class Op(C.Structure):
    """dasr_op: one recorded launch.  OP_CONV carries a ConvParams; every other kind passes its arguments in the untyped slots i / f / l / p / t,
    laid out by OP_ARGS (build with make_op, read and patch with get / set)."""
    _fields_ = [('op', c_i32), ('i', c_i32 * 8), ('f', c_f32 * 4), ('l', c_i64 * 4), ('p', c_vp * 4), ('t', Tensor * 5),
                ('conv', ConvParams), ('flops', C.c_double), ('bytes', C.c_double)]

    def get(self, name):
        """the argument `name` of this op (OP_ARGS)"""
        arr, k, enc = _slot(self.op, name)
        a = getattr(self, arr)
        if enc == '*':
            return list(a) if arr == 'f' else list((c_f32 * 4).from_buffer(a))
        if enc == 'f':
            return struct.unpack('<f', struct.pack('<I', a[k] & 0xffffffff))[0]
        return a[k]

    def set(self, name, value):
        """write the argument `name` of this op (OP_ARGS); None / NULL_T are the zero bytes an argument left out has"""
        arr, k, enc = _slot(self.op, name)
        a = getattr(self, arr)
        if enc == '*':
            if arr == 'f':
                a[:] = [float(v) for v in value]
            else:
                (c_f32 * 4).from_buffer(a)[:] = [float(v) for v in value]
        elif enc == 'f':
            a[k] = struct.unpack('<I', struct.pack('<f', value))[0]
        elif value is None:
            a[k] = Tensor(None, 0, 0) if arr == 't' else 0
        else:
            a[k] = value


OP_CONV, OP_WGRAD, OP_WGRAD_REDUCE, OP_PACK, OP_DOWNSUM, OP_AXPBY, OP_FILL, OP_L1LOSS, OP_NCHW2B, OP_B2NCHW = range(1, 11)
(OP_INORM_FWD, OP_INORM_BWD, OP_BCE, OP_DWT_FWD, OP_DWT_BWD, OP_LOWPASS, OP_MAXPOOL, OP_MAXPOOL_BWD, OP_L1DIFF, OP_AFFINE4,
 OP_BILINEAR, OP_LOGLOSS, OP_SIGMOID_BWD, OP_PRELU_GRAD, OP_LOWPASS_VALID, OP_ADD_FLAT, OP_SIGMOID_FWD, OP_EVENT_RECORD, OP_STREAM_WAIT,
 OP_SET_STREAM) = range(11, 31)
OP_CVT_F16, OP_DOWNSUM_F16, OP_PIXSHUF, OP_PIXUNSHUF = 31, 32, 33, 34
OP_LPIPS_S2D, OP_MAXPOOL3, OP_MAXPOOL3_BWD, OP_LPIPS_HEAD, OP_RAGAN = 35, 36, 37, 38, 39
OP_BNORM_FWD, OP_BNORM_BWD, OP_BNORM_RUNNING = 40, 41, 42
OP_DDM_SPREAD = 43
OP_INORM_JVP, OP_INORM_SECOND, OP_GRAD_PENALTY, OP_FILL_SCALED = 44, 45, 46, 47
OP_CONV_CHAIN = 48
OP_RDB_CHAIN = 49
OP_BNORM_JVP, OP_BNORM_SECOND = 50, 51   # --wgan with BatchNorm discriminators (round 6)
OP_PRELU_FINAL = 52
OP_RESBLOCK = 53   # fused residual block of SRResNet (ABI 21)
OP_LPIPS_S2D_ANY = 54   # LPIPS input stage at any image size (the folder evaluator)

# Argument slots of every op kind the plan builders record (all but OP_CONV), by the parameter name of the entry point that dasr_run_ops
# (csrc/misc.hip) passes the slot to.  Slot codes: i0..i6 int32, f0..f3 float, l0..l3 int64, p0..p3 pointer, t0..t4 dasr_tensor;
# 'f*': four floats in f[0..3]; 'l*': four floats in the first 16 bytes of l; 'l1f' / 'l2f': a float's bits in the low half of l[1] / l[2].
# i[7] of every kind is 'tag', the time bucket of OpList.tag (no kernel reads it).  tests/test_host.py checks the table against the switch.
OP_ARGS = {
    OP_WGRAD: dict(parts_dev='p0', nparts='i0', nsplit='i1', kh='i2', stride='i3', f32='i4', ws='p1'),
    # scale x inv_prescale (when non-zero) is the reduce scale: inv_prescale undoes the f16 operand pre-scale
    OP_WGRAD_REDUCE: dict(parts_dev='p0', nparts='i0', ws='p1', grad_flat='p2', scale='f0', inv_prescale='f1', few_splits='i1'),
    OP_PACK: dict(descs_dev='p0', ndesc='i0', total_pieces='l0', piece_prefix_dev='p1', params_flat='p2', packed='p3'),
    OP_DOWNSUM: dict(src='t0', N='i0', C='i1', H='i2', W='i3', mask='t1', mask_f32='i4', slope='f0', dst_f32='t2', dst_bf16='t3'),
    OP_AXPBY: dict(x='t0', a='f0', z='t1', b='f1', N='i0', C='i1', H='i2', W='i3', out_f32='t2', out_bf16='t3', gamma='f2', mask='t4', slope='f3',
                   slope_ptr='p0'),
    OP_FILL: dict(p='p0', n='l0', value='f0'),
    OP_L1LOSS: dict(sr='t0', hr_nchw='p0', weight_map='p1', N='i0', C='i1', H='i2', W='i3', coef='f0', loss_acc='p2', grad='t1', accumulate='i4',
                    grad_scale='f1'),
    OP_NCHW2B: dict(src='p0', N='i0', C='i1', H='i2', W='i3', dst_f32='t0', dst_bf16='t1'),
    OP_B2NCHW: dict(src='t0', N='i0', C='i1', H='i2', W='i3', dst='p0'),
    OP_INORM_FWD: dict(x='t0', N='i0', C='i1', H='i2', W='i3', eps='f0', slope='f1', y='t1', stats='p0'),
    OP_INORM_BWD: dict(a='t0', ga='t1', N='i0', C='i1', H='i2', W='i3', slope='f0', stats='p0', gx='t2'),
    OP_BCE: dict(x='t0', N='i0', C='i1', H='i2', W='i3', gan_type='i4', target='f0', coef='f1', gcoef='f2', loss_acc='p0', score_acc='p1',
                 score_coef='f3', grad='t1'),
    OP_DWT_FWD: dict(x='t0', N='i0', C='i1', H2='i2', W2='i3', norm='i4', ll='t1', hc='t2'),
    OP_DWT_BWD: dict(gll='t0', ghc='t1', N='i0', C='i1', H2='i2', W2='i3', norm='i4', gx='t2', accumulate='i5'),
    OP_LOWPASS: dict(x='t0', x2='t1', w='p0', k='i4', N='i0', C='i1', H='i2', W='i3', mode='i5', a_h='f0', b_h='f1', out_low='t2', out_high='t3',
                     accumulate='i6'),
    OP_MAXPOOL: dict(x='t0', is_f32='i4', N='i0', C='i1', Ho='i2', Wo='i3', y='t1', Win='i6'),
    OP_MAXPOOL_BWD: dict(x='t0', gy='t1', is_f32='i4', N='i0', C='i1', Ho='i2', Wo='i3', gx='t2', relu_mask='i5', Win='i6'),
    OP_L1DIFF: dict(a='t0', b='t1', is_f32='i4', N='i0', C='i1', H='i2', W='i3', coef='f0', gcoef='f1', loss_acc='p0', ga='t2'),
    OP_AFFINE4: dict(x='t0', N='i0', C='i1', H='i2', W='i3', scale4='f*', shift4='l*', y='t1', y_f32='i4', accumulate='i5'),
    OP_BILINEAR: dict(src='p0', N='i0', h='i1', w='i2', factor='i3', dst='p1'),
    OP_LOGLOSS: dict(x='t0', N='i0', H='i1', W='i2', mode='i3', eps='f0', coef='f1', gcoef='f2', loss_acc='p0', score_acc='p1', score_coef='f3',
                     grad='t1', accumulate='i4'),
    OP_SIGMOID_BWD: dict(y='t0', g='t1', N='i0', C='i1', H='i2', W='i3', gz='t2'),
    # f16 != 0: dasr_prelu_grad_f16 (y and gx f16, gx pre-scaled by 1 / inv_prescale; scale x inv_prescale when that is non-zero)
    OP_PRELU_GRAD: dict(y='t0', gx='t1', N='i0', C='i1', H='i2', W='i3', slope='p0', scratch256='p1', dst='p2', scale='f0', f16='i4', inv_prescale='f1'),
    OP_LOWPASS_VALID: dict(x='t0', w='p0', k='i4', N='i0', C='i1', H='i2', W='i3', mode='i5', out='t1', accumulate='i6'),
    OP_ADD_FLAT: dict(y='p0', x='p1', n='l0'),
    OP_SIGMOID_FWD: dict(x='t0', N='i0', C='i1', H='i2', W='i3', y='t1'),
    OP_EVENT_RECORD: dict(event='p0'),
    OP_STREAM_WAIT: dict(event='p0'),
    OP_SET_STREAM: dict(stream='p0'),   # null: back to the stream dasr_run_ops was called with
    OP_PIXSHUF: dict(src='t0', N='i0', C4='i1', H='i2', W='i3', dst='t1'),
    OP_PIXUNSHUF: dict(gsrc='t0', mask='t1', slope='f0', N='i0', C4='i1', H='i2', W='i3', gdst='t2'),
    # form selects the entry point: 0 dasr_cvt_f16, 1 / 2 dasr_cvt_split16 (f16 / bf16), 3 dasr_f16_residual
    OP_CVT_F16: dict(x='t0', N='i0', C='i1', H='i2', W='i3', scale='f0', y='t1', form='i4'),
    OP_DOWNSUM_F16: dict(src='t0', N='i0', C='i1', H='i2', W='i3', mask='t1', slope='f0', out_scale='f1', dst_f32='t2', dst_f16='t3'),
    OP_BNORM_FWD: dict(x='t0', N='i0', C='i1', H='i2', W='i3', group='i4', eps='f0', slope='f1', gamma='p0', beta='p1', y='t1', stats='p2'),
    OP_BNORM_BWD: dict(x='t0', ga='t1', N='i0', C='i1', H='i2', W='i3', group='i4', slope='f0', gamma='p0', beta='p1', stats='p2', gx='t2', dgamma='p3',
                       dbeta='l0', pscale='f1'),   # dbeta: a device address
    OP_BNORM_RUNNING: dict(stats='p0', g='i0', C='i1', count='i2', momentum='f0', running_mean='p1', running_var='p2', num_batches_tracked='p3'),
    OP_INORM_JVP: dict(a='t0', t='t1', N='i0', C='i1', H='i2', W='i3', slope='f0', stats='p0', out='t2'),
    OP_INORM_SECOND: dict(a='t0', t='t1', ga='t2', N='i0', C='i1', H='i2', W='i3', slope='f0', stats='p0', out='t3', accumulate='i4'),
    OP_RESBLOCK: dict(p='p0'),
    OP_PRELU_FINAL: dict(partial='p0', nblocks='i0', stride='l0', count='i1', slopes='p1', dsts='p2', scale='f0'),
    OP_BNORM_JVP: dict(x='t0', t='t1', N='i0', C='i1', H='i2', W='i3', group='i4', slope='f0', gamma='p0', beta='p1', stats='p2', out='t2'),
    OP_BNORM_SECOND: dict(x='t0', t='t1', ga='t2', N='i0', C='i1', H='i2', W='i3', group='i4', slope='f0', gamma='p0', beta='p1', stats='p2', out='t3',
                          accumulate='i5', dgamma='p3', pscale='f1'),
    OP_GRAD_PENALTY: dict(g='t0', N='i0', C='i1', H='i2', W='i3', weight='f0', part256='p0', out3='p1', loss_acc='p2', stage='i4',
                          world='i5'),   # world 0 is read as 1
    OP_FILL_SCALED: dict(x='t0', N='i0', C='i1', H='i2', W='i3', scalar='p0', factor='f0'),
    OP_CONV_CHAIN: dict(dev_layers='p0', host_layers='p1', dev_dep_chunk='p2', nlayers='i0', dev_flags='p3', dev_err='l0'),   # dev_err: a device address
    OP_RDB_CHAIN: dict(dev_layers='p0', host_layers='p1', nlayers='i0', dev_flags='p3', dev_err='l0'),
    OP_DDM_SPREAD: dict(d='t0', N='i0', n_h='i1', n_w='i2', H='i3', W='i4', jump='i5', rf='i6', start='f0', out='t1'),
    OP_RAGAN: dict(a='t0', b='t1', N='i0', H='i1', W='i2', stage='i3', n_glob='i4', form='i5', ta='f0', tb='f1', coef='f2', gcoef='f3', eps='l2f',
                   sums='p0', part='p1', loss_acc='p2', score_a='p3', score_b='l0', score_coef='l1f', ga='t2', gb='t3'),   # score_b: a device address
    OP_LPIPS_S2D: dict(x='t0', N='i0', H='i1', W='i2', scale4='f*', shift4='l*', y='t1', mode='i3'),
    OP_MAXPOOL3: dict(x='t0', N='i0', C='i1', H='i2', W='i3', y='t1'),
    OP_MAXPOOL3_BWD: dict(x='t0', gy='t1', N='i0', C='i1', H='i2', W='i3', gx='t2', relu_mask='i4', accumulate='i5'),
    OP_LPIPS_HEAD: dict(f='t0', pair_off='l0', N='i0', C='i1', H='i2', W='i3', lin='p0', eps='f0', coef='f1', gcoef='f2', loss_acc='p1', g0='t1',
                        relu_mask='i4'),
    OP_LPIPS_S2D_ANY: dict(x='t0', N='i0', H='i1', W='i2', scale4='f*', shift4='l*', y='t1'),
}


def _slot(kind, name):
    """(slot array, index, encoding) of argument `name` of op kind `kind`: 'i3' -> ('i', 3, ''), 'f*' -> ('f', 0, '*'), 'l2f' -> ('l', 2, 'f')"""
    code = 'i7' if name == 'tag' else OP_ARGS.get(kind, {}).get(name)
    if code is None:
        raise TypeError('op kind %d has no argument %r' % (kind, name))
    if code[1] == '*':
        return code[0], 0, '*'
    return code[0], int(code[1]), code[2:]


def make_op(kind, flops=0.0, bytes=0.0, **args):
    """an Op of `kind` with the named arguments of OP_ARGS (and 'tag'); arguments left out are zero"""
    o = Op()
    o.op = kind
    o.flops, o.bytes = flops, bytes
    for name, v in args.items():
        o.set(name, v)
    return o

_SIGS = {
    'dasr_conv': [C.POINTER(ConvParams), c_vp],
    'dasr_conv_chain': [c_vp, C.POINTER(ConvParams), c_vp, c_i32, c_vp, c_vp, c_vp],
    'dasr_rdb_chain': [c_vp, C.POINTER(ConvParams), c_i32, c_vp, c_vp, c_vp],
    'dasr_conv_naive': [C.POINTER(ConvParams), c_vp, c_vp],
    'dasr_resblock': [C.POINTER(ResblockParams), c_vp],
    'dasr_set_tuning': [c_i32, c_i32],
    'dasr_wgrad': [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp],
    'dasr_wgrad_set_mode': [c_i32],
    'dasr_wgrad_reduce': [c_vp, c_i32, c_vp, c_vp, c_f32, c_i32, c_vp],
    'dasr_pack_weights': [c_vp, c_i32, c_i64, c_vp, c_vp, c_vp, c_vp],
    'dasr_nchw_to_blocked': [c_vp, c_i32, c_i32, c_i32, c_i32, Tensor, Tensor, c_vp],
    'dasr_blocked_to_nchw': [Tensor, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp],
    'dasr_l1_loss': [Tensor, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, Tensor, c_i32, c_f32, c_vp],
    'dasr_pixel_shuffle_f16': [Tensor, c_i32, c_i32, c_i32, c_i32, Tensor, c_vp],
    'dasr_pixel_unshuffle_f16': [Tensor, Tensor, c_f32, c_i32, c_i32, c_i32, c_i32, Tensor, c_vp],
    'dasr_cvt_f16': [Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, Tensor, c_vp],
    'dasr_cvt_split16': [Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, Tensor, c_i32, c_vp],
    'dasr_f16_residual': [Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, Tensor, c_vp],
    'dasr_downsum2x_f16': [Tensor, c_i32, c_i32, c_i32, c_i32, Tensor, c_f32, c_f32, Tensor, Tensor, c_vp],
    'dasr_downsum2x': [Tensor, c_i32, c_i32, c_i32, c_i32, Tensor, c_i32, c_f32, Tensor, Tensor, c_vp],
    'dasr_axpby': [Tensor, c_f32, Tensor, c_f32, c_i32, c_i32, c_i32, c_i32, Tensor, Tensor, c_f32, Tensor, c_f32, c_vp, c_vp],
    'dasr_adam': [c_vp, c_vp, c_vp, c_vp, c_i64, c_f32, c_f32, c_f32, c_f32, c_f32, c_i32, c_vp, c_vp, c_vp],
    'dasr_fill_f32': [c_vp, c_i64, c_f32, c_vp],
    'dasr_add_flat': [c_vp, c_vp, c_i64, c_vp],
    'dasr_inorm_lrelu_fwd': [Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, Tensor, c_vp, c_vp],
    'dasr_inorm_lrelu_bwd': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, Tensor, c_vp],
    'dasr_inorm_lrelu_jvp': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, Tensor, c_vp],
    'dasr_inorm_second': [Tensor, Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, Tensor, c_i32, c_vp],
    'dasr_grad_penalty': [Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_i32, c_i32, c_vp],
    'dasr_fill_scaled': [Tensor, c_i32, c_i32, c_i32, c_i32, c_vp, c_f32, c_vp],
    'dasr_bce_logits': [Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp, c_f32, Tensor, c_vp],
    'dasr_gan_loss': [Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp, c_f32, Tensor, c_vp],
    'dasr_dwt_fwd': [Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, Tensor, Tensor, c_vp],
    'dasr_dwt_bwd': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, Tensor, c_i32, c_vp],
    'dasr_lowpass': [Tensor, Tensor, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, Tensor, Tensor, c_i32, c_vp],
    'dasr_maxpool2': [Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, Tensor, c_i32, c_vp],
    'dasr_maxpool2_bwd': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, Tensor, c_i32, c_i32, c_vp],
    'dasr_l1_diff': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_vp, Tensor, c_vp],
    'dasr_affine4': [Tensor, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, Tensor, c_i32, c_i32, c_vp],
    'dasr_bilinear_up': [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp],
    'dasr_logloss': [Tensor, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_vp, c_vp, c_f32, Tensor, c_i32, c_vp],
    'dasr_sigmoid_bwd': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, Tensor, c_vp],
    'dasr_sigmoid_fwd': [Tensor, c_i32, c_i32, c_i32, c_i32, Tensor, c_vp],
    'dasr_gather_crops': [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp],
    'dasr_event_create': [],
    'dasr_event_destroy': [c_vp],
    'dasr_prelu_grad': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_f32, c_vp],
    'dasr_prelu_grad_f16': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_f32, c_vp],
    'dasr_lowpass_valid': [Tensor, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, Tensor, c_i32, c_vp],
    'dasr_run_ops': [c_vp, c_i32, c_vp],
    'dasr_run_ops_mt': [c_vp, c_vp, c_vp, c_i32],
    'dasr_last_failed_op': [],
    'dasr_ddm_spread': [Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, Tensor, c_vp],
    'dasr_abi_version': [],
    'dasr_prof_filter': [C.c_char_p],
    'dasr_red_release': [],
    'dasr_probe_tr16': [c_vp],
    'dasr_rccl_unique_id': [c_vp],
    'dasr_rccl_init': [c_vp, c_i32, c_i32, c_vp],
    'dasr_allreduce': [c_vp, c_vp, c_i64, c_vp],
    'dasr_broadcast': [c_vp, c_vp, c_i64, c_i32, c_vp],
    'dasr_rccl_destroy': [c_vp],
    'dasr_bnorm_lrelu_fwd': [Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_vp, c_vp, Tensor, c_vp, c_vp],
    'dasr_prelu_final': [c_vp, c_i32, c_i64, c_i32, c_vp, c_vp, c_f32, c_vp],
    'dasr_bnorm_lrelu_jvp': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, Tensor, c_vp],
    'dasr_bnorm_second': [Tensor, Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, Tensor, c_i32, c_vp, c_f32, c_vp],
    'dasr_bnorm_lrelu_bwd': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, Tensor, c_vp, c_vp, c_f32, c_vp],
    'dasr_bnorm_running': [c_vp, c_i32, c_i32, c_i32, c_f32, c_vp, c_vp, c_vp, c_vp],
    'dasr_ragan': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_f32, c_f32, c_f32, c_f32, c_vp, c_vp, c_vp, c_vp, c_vp, c_f32, Tensor, Tensor, c_vp],
    'dasr_lpips_s2d': [Tensor, c_i32, c_i32, c_i32, c_vp, c_vp, Tensor, c_i32, c_vp],
    'dasr_lpips_s2d_any': [Tensor, c_i32, c_i32, c_i32, c_vp, c_vp, Tensor, c_vp],
    'dasr_maxpool3s2': [Tensor, c_i32, c_i32, c_i32, c_i32, Tensor, c_vp],
    'dasr_maxpool3s2_bwd': [Tensor, Tensor, c_i32, c_i32, c_i32, c_i32, Tensor, c_i32, c_i32, c_vp],
    'dasr_lpips_head': [Tensor, c_i64, c_i32, c_i32, c_i32, c_i32, c_vp, c_f32, c_f32, c_f32, c_vp, Tensor, c_i32, c_vp],
    'dasr_img_ws_bytes': [c_i32, c_i32, c_i32, c_i32, c_i32],
    'dasr_tensor2img_u8': [c_vp, c_i32, c_i32, c_i32, c_i32, C.c_double, C.c_double, c_vp, c_vp, c_vp, c_vp],
    'dasr_img_sse': [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_i64, c_vp],
    'dasr_img_ssim': [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp],
    'dasr_img_ssim_box': [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp],
    'dasr_img_channel_sums': [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_i64, c_vp],
    'dasr_u8_to_planar': [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp],
    'dasr_imresize_down': [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'dasr_gather_crops_u8': [c_vp, c_i32, c_i32, c_vp, c_vp],
    'dasr_crops_bicubic_down': [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp],
    'dasr_gather_srn_u8': [c_vp, c_i32, c_i32, c_vp],
    'dasr_crops_down4_u8': [c_vp, c_vp, c_i32, c_i32, c_vp, c_vp],
    'dasr_dihedral8': [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp],
    'dasr_dihedral8_mean': [c_vp, c_vp, c_i32, c_i32, c_i32, c_vp, c_vp],
    'dasr_bp_residual': [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'dasr_bp_update': [c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'dasr_windows_down_u8': [c_vp, c_i32, c_i32, c_vp, c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp],
    'dasr_imresize_up': [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp, c_vp, c_i32, c_vp],
    'dasr_jpeg_blocks': [c_vp, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp],
    'dasr_jpeg_merge': [c_vp, c_i32, c_i32, c_i32, c_vp, c_vp],
    'dasr_noise_u8': [c_vp, c_vp, c_i32, c_i64, C.c_double, c_i64, c_i64, c_vp],
    'dasr_png_filter': [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp],
    'dasr_png_codes': [c_vp, c_i32, c_vp, c_vp, c_vp, c_vp],
    'dasr_png_emit': [c_vp, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_vp, c_vp, c_i64, c_vp, c_vp, c_vp],
    'dasr_png_pack': [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_vp],
    'dasr_png_filter_fmt': [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_i64, c_vp, c_vp, c_i32, c_vp],
    'dasr_png_pack_fmt': [c_vp, c_vp, c_i32, c_vp, c_vp, c_i32, c_vp, c_vp, c_i64, c_vp, c_vp, c_i64, c_vp, c_i32, c_vp],
    'dasr_prof_begin': [c_i32],
    'dasr_prof_end': [c_i32, c_vp, c_vp, c_vp, c_vp, c_vp],
}

# micro-benchmark probes: libdasr_bench.so (include/dasr_hip_bench.h), never part of the product library
_BENCH_SIGS = {
    'dasr_probe_mfma_data': [c_i32, c_i32, c_vp, c_vp],
    'dasr_probe_tile_sync': [c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp, c_vp, c_vp],
    'dasr_probe_mfma_peak': [c_i32, c_vp, c_vp],
    'dasr_probe_spin': [c_i32, c_i32, c_vp],
    'dasr_probe_store': [c_vp, c_i32, c_i32, c_i32, c_i32, c_i32, c_vp, c_vp],
}
BENCH_LIB_PATH = os.path.join(HERE, 'libdasr_bench.so')

ABI_VERSION = 22
_lib = None
_bench = None


def bench_lib():
    """the probe library (bench.py, scripts/micro_*.py); raises when it has not been built (`python -m dasr_amd.build --bench`)"""
    global _bench
    if _bench is None:
        if not os.path.exists(BENCH_LIB_PATH):
            raise DasrHipError('libdasr_bench.so is missing (%s): run `python -m dasr_amd.build --bench`' % BENCH_LIB_PATH)
        import torch  # noqa: F401  (same HIP runtime as torch, see lib())
        L = C.CDLL(BENCH_LIB_PATH)
        for name, args in _BENCH_SIGS.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = c_i32
        _bench = L
    return _bench


class DasrHipError(RuntimeError):
    pass


def exported_symbols():
    """Names every entry point include/dasr_hip.h declares (used by the CPU symbol test)."""
    return sorted(_SIGS)


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DasrHipError('libdasr_hip.so is missing (%s): run `python -m dasr_amd.build` or __graft_entry__.build(); '
                               'the DASR MI355X path has no fallback.' % LIB_PATH)
        # torch first: its wheel bundles its own libamdhip64.so (SONAME libamdhip64.so.7, but NEEDED as "libamdhip64.so"); if this library is
        # loaded before torch, /opt/rocm's runtime comes in with it and torch then maps a SECOND HIP runtime -- torch's streams and
        # allocations are foreign to ours and the first launch fails (hipErrorNoDevice).  With torch loaded, our NEEDED
        # libamdhip64.so.7 resolves by SONAME to the runtime torch uses.  (A C consumer without torch gets /opt/rocm's, alone.)
        import torch  # noqa: F401
        L = C.CDLL(os.environ.get('DASR_HIP_LIB') or LIB_PATH)  # DASR_HIP_LIB: instrumented build for scripts/ (same ABI)
        for name, args in _SIGS.items():
            fn = getattr(L, name)  # AttributeError if the library does not export it
            fn.argtypes = args
            fn.restype = c_vp if name == 'dasr_event_create' else c_i32
        if L.dasr_abi_version() != ABI_VERSION:
            raise DasrHipError('libdasr_hip.so ABI %d != binding ABI %d; rebuild' % (L.dasr_abi_version(), ABI_VERSION))
        for kv in [x for x in os.environ.get('DASR_TUNE', '').split(',') if x]:   # A/B of kernel variants without code changes: DASR_TUNE="2=12"
            k, v = kv.split('=')
            if L.dasr_set_tuning(int(k), int(v)) != 0:
                raise DasrHipError('DASR_TUNE: bad tuning key/value %r' % kv)
        _lib = L
    return _lib


def check(rc, what=''):
    if rc != 0:
        raise DasrHipError('%s failed with code %d' % (what or 'dasr call', rc))

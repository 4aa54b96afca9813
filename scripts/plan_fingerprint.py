"""Fingerprint of the RECORDED plans of the GAN trainers, and of two training steps: what a host-side change of the plan builders must leave alone.

    python scripts/plan_fingerprint.py [--root DIR]             one line per op list of every configuration below (needs a GPU: the models build there)
    python scripts/plan_fingerprint.py --steps 2 [--root DIR]   two seeded steps of four configurations: parameters and logged values, bit for bit
    python scripts/plan_fingerprint.py --vgg [--root DIR]       the VGG19-34 / VGG16-30 plans in every precision, recorded on the host (no GPU, no library)

--root DIR: the directory whose `dasr_amd` package is fingerprinted (default: this checkout), e.g. an export of another commit with its built library.
The script reads plans only through OpList.ops, _lib.Op and _lib.OP_ARGS, so the same file runs on both sides of a refactor; equal output = equal
launches.  Lines that start with '#' (build times) are not part of the comparison.

Canonical form of an op list: per op, in order, the kind and every slot of dasr_op.  Non-pointer slots bit for bit (floats as hex).  Pointers -- the p
slots, tensor bases, the pointer fields of dasr_conv_params, and the l slots OP_ARGS documents as device addresses -- as (rank of the allocation by
first appearance, byte offset inside it): the allocations are the storages of every torch tensor reachable from the model (plans, networks, ParamStores,
pack buffers, OpList.keep), so two processes agree and a wrong offset inside an allocation changes the hash.  A pointer into no tensor (a ctypes
table on the host, a stream, an event) gets a rank of its own kind by first appearance.  The parameter blocks behind a chained-conv op, the host part
tables of the weight-gradient groups a list keeps and the op indices the trainers address (mix_op, cut, sym_ops, ragan cuts) are hashed too.  One rank
table per configuration, filled in the order the lists are printed, so an aliasing between two lists is part of the fingerprint."""
import argparse
import bisect
import ctypes as C
import hashlib
import os
import random
import sys
import time
import types

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

L_POINTERS = ('dbeta', 'dev_err', 'score_b')   # the int64 slots OP_ARGS documents as device addresses


class Canon:
    def __init__(self, _lib, roots):
        import torch
        self.L = _lib
        allocs, seen, stack, hold = {}, set(), list(roots), []
        while stack:
            o = stack.pop()
            if id(o) in seen or isinstance(o, (str, bytes, int, float, bool, type(None), C.Structure, C.Array, C._SimpleCData)):
                continue
            seen.add(id(o))
            hold.append(o)
            if isinstance(o, torch.Tensor):
                st = o.untyped_storage()
                if st.nbytes():
                    allocs[st.data_ptr()] = max(allocs.get(st.data_ptr(), 0), st.nbytes())
            elif isinstance(o, dict):
                stack.extend(o.keys())
                stack.extend(o.values())
            elif isinstance(o, (list, tuple, set, frozenset)):
                stack.extend(o)
            elif isinstance(o, types.MethodType):
                stack.append(o.__self__)
            elif isinstance(o, types.FunctionType):
                for cell in o.__closure__ or ():
                    try:
                        stack.append(cell.cell_contents)
                    except ValueError:   # an empty cell
                        pass
            elif type(o).__module__.split('.')[0] == 'dasr_amd':
                stack.extend(getattr(o, '__dict__', {}).values())
                stack.extend(getattr(o, s) for s in getattr(type(o), '__slots__', ()) if hasattr(o, s))
        self.starts = sorted(allocs)
        self.sizes = [allocs[s] for s in self.starts]
        self.rank, self.host = {}, {}
        self.lptr = {}
        for kind, args in _lib.OP_ARGS.items():
            self.lptr[kind] = {int(code[1]) for name, code in args.items() if name in L_POINTERS and code[0] == 'l' and len(code) == 2}

    def ptr(self, p):
        if not p:
            return 0
        i = bisect.bisect_right(self.starts, p) - 1
        if i >= 0 and p < self.starts[i] + self.sizes[i]:
            return ('d', self.rank.setdefault(self.starts[i], len(self.rank)), p - self.starts[i])
        return ('h', self.host.setdefault(p, len(self.host)))

    def struct(self, s, lptr=()):
        T = self.L.Tensor
        out = []
        for name, typ in s._fields_:
            v = getattr(s, name)
            if typ is T:
                out.append((self.ptr(v.p), v.n_stride, v.cb_stride))
            elif typ is C.c_void_p:
                out.append(self.ptr(v))
            elif issubclass(typ, C.Array):
                if typ._type_ is T:
                    out.append([(self.ptr(t.p), t.n_stride, t.cb_stride) for t in v])
                elif typ._type_ is C.c_void_p:
                    out.append([self.ptr(x) for x in v])
                elif typ._type_ in (C.c_float, C.c_double):
                    out.append([float(x).hex() for x in v])
                elif name == 'l':
                    out.append([self.ptr(x) if i in lptr else int(x) for i, x in enumerate(v)])
                else:
                    out.append([int(x) for x in v])
            elif issubclass(typ, C.Structure):
                out.append(self.struct(v))
            elif typ in (C.c_float, C.c_double):
                out.append(float(v).hex())
            else:
                out.append(int(v))
        return out

    def oplist(self, ol):
        L = self.L
        chains = {k for k in (getattr(L, 'OP_CONV_CHAIN', None), getattr(L, 'OP_RDB_CHAIN', None)) if k is not None}
        out = []
        for o in ol.ops:
            out.append(self.struct(o, self.lptr.get(o.op, ())))
            if o.op in chains and o.get('host_layers'):   # the parameter blocks of a chained launch (host copy of the device table)
                arr = (L.ConvParams * o.get('nlayers')).from_address(o.get('host_layers'))
                out.append([self.struct(p) for p in arr])
        for grp in getattr(ol, 'keep', ()):   # weight-gradient groups: their host part tables
            if not hasattr(grp, 'parts'):
                continue
            out.append([getattr(grp, a, None) for a in ('kh', 'stride', 'nsplit', 'ws_floats', 'n_red', 'ppu')])
            for entry in grp.parts:
                row = []
                for e in entry:
                    if isinstance(e, C.Structure):
                        row.append(self.struct(e))
                    elif isinstance(e, list):   # WgradGroup3: [(oc tile, reduce description)]
                        row.append([(ot, sorted(t.items())) for ot, t in e])
                    else:
                        row.append(e)
                out.append(row)
        return hashlib.sha256(repr(out).encode()).hexdigest()


def emit(name, canon, lists, indices=()):
    for ln, ol in lists:
        if ol is None:
            print('plan|%s|%s|absent' % (name, ln))
        else:
            print('plan|%s|%s|%d|%s' % (name, ln, len(ol.ops), canon.oplist(ol)))
    for k, v in indices:
        print('idx|%s|%s|%r' % (name, k, v))
    print('ptrs|%s|allocations %d host %d' % (name, len(canon.rank), len(canon.host)))
    sys.stdout.flush()


def seed_all(torch, s=0):
    import numpy as np
    torch.manual_seed(s)
    np.random.seed(s)
    random.seed(s)


SRN_CASES = ['dasr_wavelet_nf32_nb2_n2_32', 'dasr_gau9_nf64_nb1_n1_32', 'dasr_srcD_wavelet_nf32_nb2_n2_32', 'dasr_srcVGG128_gau5_nf32_nb1_n3_32',
             'dasr_ragan_wavelet_nf32_nb1_n3_32', 'dasr_lpips_wavelet_nf32_nb2_n2_32', 'dasr_wgan_gau9_nf32_nb1_n2_32', 'avgpool:dasr_gau9_nf64_nb1_n1_32']
SRN_STEP_CASES = ['dasr_srcVGG128_gau5_nf32_nb1_n3_32', 'dasr_ragan_wavelet_nf32_nb1_n3_32']


def srn_model(case):
    from oracle import fixtures
    from dasr_amd import options
    from dasr_amd.models import create_model
    base = case.split(':')[-1]
    opt = fixtures.make_opt(base)
    opt['gpu_ids'] = [0]
    opt['train']['vgg_seed'] = 77
    if case.startswith('avgpool:'):   # the gau9 fixture with the box filter (`norm` is on in every fixture)
        opt['train']['fs'] = 'avgpool'
    return create_model(options.dict_to_nonedict(opt)), fixtures.CASES[base], base


def srn_plans(torch):
    for case in SRN_CASES:
        seed_all(torch)
        m, c, _ = srn_model(case)
        P = m._plan(c['n'], c['lr'], c['lr'])
        lists = [('fwd', P.fwd), ('g_loss_bwd', P.g_loss_bwd), ('d_step', P.d_step), ('ds_step', P.ds_step)]
        lists += [('%s%d' % (k, i), getattr(P, k)[i]) for k in ('rg', 'rd', 'rs') for i in range(3)]
        lists += [('ds_run_g', P.ds_run_g), ('ds_run_d', P.ds_run_d)]
        emit('srn/' + case, Canon(_LIB, [m, P]), lists)
        del m, P
        torch.cuda.empty_cache()


def dsn_opts(**kw):
    o = dict(kernel_size=5, n_res_blocks=2, w_per=0.01, vgg_seed=78, per_type='VGG', allow_random_perceptual=True)
    o.update(kw)
    return o


def dsn_configs():
    out = []
    for filt, cs in (('gau', 'cat'), ('avg_pool', 'cat'), ('wavelet', 'cat'), ('wavelet', 'sum')):
        for norm in ('Instance', 'Batch'):
            for loss, kw in (('plain', {}), ('ragan', dict(ragan=True)), ('wgan', dict(wgan=True))):
                out.append(('dsn/fsd_%s_%s_%s_%s' % (filt, cs, norm, loss), dsn_opts(filter=filt, cat_or_sum=cs, norm_layer=norm, **kw), (2, 128, 128)))
    out.append(('dsn/nld_s2_wavelet_Batch_wgan', dsn_opts(filter='wavelet', norm_layer='Batch', wgan=True, discriminator='nld_s2'), (2, 128, 128)))
    out.append(('dsn/nld_s1_gau', dsn_opts(filter='gau', discriminator='nld_s1'), (2, 128, 128)))
    out.append(('dsn/dsgan_gau', dsn_opts(filter='gau', generator='DSGAN'), (2, 128, 128)))
    out.append(('dsn/lpips_rot_flip_gau', dsn_opts(filter='gau', per_type='LPIPS', lpips_rot_flip=True), (2, 256, 256)))
    return out


def dsn_plans(torch):
    from dasr_amd.dsn_model import DSNModel, _InferPlan
    for name, opt, (N, H, W) in dsn_configs():
        seed_all(torch)
        m = DSNModel(opt, device='cuda')
        t0 = time.perf_counter()
        P = m._plan(N, H, W)
        dt = time.perf_counter() - t0
        gp = P.gp
        lists = [('fwd', P.fwd), ('d_bwd', P.d_bwd), ('g_bwd', P.g_bwd), ('d_running', P.d_running), ('gp.ops', gp.ops if gp is not None else None)]
        idx = [('mix_op', getattr(gp, 'mix_op', None)), ('cut', getattr(gp, 'cut', None)),
               ('sym_ops', [(['fwd', 'g_bwd'][lst is P.g_bwd], i, base) for lst, i, base in getattr(P, 'sym_ops', ())]),
               ('ragan_cuts_fwd', getattr(P, 'ragan_cuts_fwd', None)), ('ragan_cut_gbwd', getattr(P, 'ragan_cut_gbwd', None))]
        emit(name, Canon(_LIB, [m, P]), lists, idx)
        if name == 'dsn/fsd_gau_cat_Instance_plain':
            print('# plan build time %s: %.3f s' % (name, dt))
        del m, P, gp
        torch.cuda.empty_cache()
    for filt in ('gau', 'wavelet'):
        seed_all(torch)
        m = DSNModel(dsn_opts(filter=filt, w_per=0.0), device='cuda')
        m.inference_discriminator()
        for kind, with_g in (('translate', True), ('ddm_of', False)):
            P = _InferPlan(m, 1, 128, 128, with_g=with_g)
            emit('infer/%s_%s' % (kind, filt), Canon(_LIB, [m, P]), [('ops', P.ops)])
        del m, P
        torch.cuda.empty_cache()


VGG_NETS = [('vgg19_34', 34, None), ('vgg16_30', 30, 'VGG16_CFG')]
VGG_PRECS = [(5, 2), (5, 5), (4, None), (3, None), (2, None), (1, None)]
VGG_SHAPES = [(3, 2, 40, 40),   # split batch; an odd 5 x 5 map in front of a pool
              (2, 2, 32, 48),   # no no-gradient half; the smallest size five pools allow
              (2, 1, 32, 32),   # the smallest size VGG16-30's five pools allow
              (2, 0, 32, 32)]   # no gradient image at all


def vgg_plans(torch):
    """the perceptual-network plans of every storage form, recorded on the host (device='cpu': no library, no GPU)"""
    from dasr_amd import gan_nets
    from dasr_amd.engine import BTensor
    for net_name, layer, cfg in VGG_NETS:
        for prec, bwd_prec in VGG_PRECS:
            for nograd in (None, '0'):
                os.environ.pop('DASR_VGG_NOGRAD_PREC', None)
                if nograd is not None:
                    os.environ['DASR_VGG_NOGRAD_PREC'] = nograd
                for mse in (False, True):
                    V = gan_nets.VGGFeatureHIP(layer, device='cpu', cfg=getattr(gan_nets, cfg) if cfg else None, prec=prec, bwd_prec=bwd_prec, mse_target=mse)
                    for N, n_g, H, W in VGG_SHAPES:
                        name = 'vgg/%s_prec%d_bwd%s_nograd%s_%s/%dx%dx%dx%d' % (net_name, prec, bwd_prec or '-', nograd or '-', 'mse' if mse else 'l1', N, n_g, H, W)
                        P = V.plan(N, n_g, H, W)
                        src = BTensor(2, 16, H, W, True, 'cpu')
                        copy = types.SimpleNamespace(ops=[P.input_copy_op(src.view(), 1, 1, H, W)])
                        gscale = getattr(P, 'gscale', None)
                        emit(name, Canon(_LIB, [V, P, src]), [('fwd', P.fwd), ('bwd', P.bwd), ('input_copy', copy)],
                             [('x_flag', P.x_flag), ('gscale', None if gscale is None else float(gscale).hex())])
    os.environ.pop('DASR_VGG_NOGRAD_PREC', None)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def steps(torch, n_steps):
    from oracle import fixtures
    for case in SRN_STEP_CASES:
        seed_all(torch)
        m, c, base = srn_model(case)
        batch = fixtures.make_batch(base)
        for step in range(1, n_steps + 1):
            m.update_learning_rate()
            m.feed_data(batch, True)
            m.optimize_parameters(step)
            log = m.get_current_log()
            print('step|srn/%s|%d|%s' % (case, step, ' '.join('%s=%s' % (k, float(v).hex()) for k, v in log.items())))
        torch.cuda.synchronize()
        for nm in ('netG', 'netD_target', 'netD_source'):
            net = getattr(m, nm, None)
            if net is not None:
                print('params|srn/%s|%s|%s' % (case, nm, sha(net.params.flat)))
                for k, b in sorted(getattr(net, 'buffers', {}).items()):
                    print('params|srn/%s|%s.%s|%s' % (case, nm, k, sha(b)))
        del m
        torch.cuda.empty_cache()
    from dasr_amd.dsn_model import DSNModel
    for name, opt in (('dsn/fsd_gau_cat_Batch_wgan', dsn_opts(filter='gau', norm_layer='Batch', wgan=True)),
                      ('dsn/fsd_wavelet_sum_Instance_plain', dsn_opts(filter='wavelet', cat_or_sum='sum', norm_layer='Instance'))):
        seed_all(torch)
        m = DSNModel(opt, device='cuda')
        g = torch.Generator().manual_seed(4321)
        hr, bic, real = torch.rand(2, 3, 128, 128, generator=g), torch.rand(2, 3, 32, 32, generator=g), torch.rand(2, 3, 32, 32, generator=g)
        hr, bic, real = hr.cuda(), bic.cuda(), real.cuda()
        for step in range(1, n_steps + 1):
            m.iteration(hr, bic, real)
            log = m.get_current_log()
            print('step|%s|%d|%s' % (name, step, ' '.join('%s=%s' % (k, float(v).hex()) for k, v in log.items())))
        torch.cuda.synchronize()
        for nm in ('netG', 'netD'):
            net = getattr(m, nm)
            print('params|%s|%s|%s' % (name, nm, sha(net.params.flat)))
            for k, b in sorted(getattr(net, 'buffers', {}).items()):
                print('params|%s|%s.%s|%s' % (name, nm, k, sha(b)))
        del m
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--root', default=REPO, help='directory of the dasr_amd package to fingerprint (default: this checkout)')
    ap.add_argument('--steps', type=int, default=0, help='run this many training steps of the four step configurations instead of hashing plans')
    ap.add_argument('--vgg', action='store_true', help='hash the perceptual-network plans of every storage form instead, recorded on the host (no GPU)')
    a = ap.parse_args()
    for p in (REPO, os.path.abspath(a.root)):   # (the oracle's fixtures come from this checkout when --root has none)
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    import torch
    import dasr_amd
    from dasr_amd import _lib
    global _LIB
    _LIB = _lib
    print('# dasr_amd from %s' % os.path.relpath(os.path.dirname(dasr_amd.__file__), REPO))
    if a.vgg:
        vgg_plans(torch)
    elif a.steps:
        steps(torch, a.steps)
    else:
        srn_plans(torch)
        dsn_plans(torch)


_LIB = None

if __name__ == '__main__':
    main()

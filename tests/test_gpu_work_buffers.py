"""The work buffers of a context as run_sequence sizes them through cosmo_pol_amd/csrc/cpol_buffers.h.

Capacities: after every library call of a few small operators, cpol_debug_read "work_buffers" equals a grow-only model of ensure()
(bytes + bytes / 8 + 256, replaced only when too small or absent) driven by this suite's own statement of the sizes
(tests/test_buffers_cpu.py: expected(), from the ENSURE lines of the parent commit), and cpol_mem_info's bytes per sub-beam gate
equal the literal sum.  The calls, at the product tests' smallest shapes: 3 rays x 65 gates of c2_rsg with one sub-beam (then 7
rays, then 3 again: nothing shrinks), with 3 sub-beams (below FORMS_RAY_PREP_MIN_SUB) and with the sub-beams of 3 x 3 Gauss-Hermite
nodes above a weight threshold of 0.75 (the centre and the four edges: the fewest from FORMS_RAY_PREP_MIN_SUB on that odd node
counts give), Doppler scheme 1; the d3_turb_motion_sub radial
(Doppler scheme 3 with broadening); a sub-beam export and the columns call of what it returned; a two-member call; a time-blended
call.

Graph replay across a regrow (CPOL_USE_GRAPH=1, device outputs): a 7-ray call with the debug reads on sizes the per-gate buffers
without the single-beam kernel's; call A (3 rays) is captured and replayed; call B (7 rays, single-beam kernel) then regrows
b_gscan alone (b_defer's 455 bytes still fit the 475 that A's 195 asked for) -- a buffer of A's sequence that the graph key did
not hold before it was made from the plan (tests/test_buffers_cpu.py has the enumeration) -- and A afterwards still gives the
bits of the plain launch sequence."""
import copy

import numpy as np
import pytest

import test_buffers_cpu as BC
import test_gpu_ensemble as E
import test_gpu_placement as P

pytestmark = pytest.mark.gpu

MIN_SUB = 4                          # FORMS_RAY_PREP_MIN_SUB (cpol_forms.h; tests/test_buffers_cpu.py checks the constant)


def n_keys_of(luts):
    return sum(int(l.value_table.shape[0]) * int(l.value_table.shape[1]) for l in luts.values())


class Watch:
    """Spies on the four entry points of a context; after each call of the library advances the model of its work buffers and
    compares it with what the context holds."""

    def __init__(self, op, luts, tag):
        self.ctx, self.tag, self.calls = op._ctx, tag, 0
        self.n_hyd, self.n_keys = len(luts), n_keys_of(luts)
        self.model = {name: 0 for name in BC.NAMES}
        assert self.ctx.work_buffers() == self.model             # a fresh context holds none
        for method in ('run_sweep', 'run_sweep_members', 'interp_subbeams', 'run_columns'):
            setattr(self.ctx, method, self.spy(method, getattr(self.ctx, method)))

    def spy(self, method, real):
        def call(p, second, *rest):
            out = real(p, second, *rest)
            self.after(method, p, second, rest)
            return out
        return call

    def after(self, method, p, second, rest):
        ctx = self.ctx
        forms = ctx.launch_forms()
        cols = second if method == 'run_columns' else None
        t = None if cols is not None else second
        timed = method == 'run_sweep_members' and t.time_blend != 0
        n_members = len(rest[0]) if method == 'run_sweep_members' and not timed else 1
        dop = p.simulate_doppler
        ray_prep = p.n_sub >= MIN_SUB and cols is None
        ml = (cols.wgate if cols is not None else t.sub_smooth) is not None
        given = [False] * 6
        if cols is not None:
            melt = cols.q_melt is not None
            given = [cols.mask is not None, cols.elev is not None, ml, melt, melt and cols.fw_melt is not None,
                     melt and cols.has_melting is not None]
        flags = (int(ml) << 1 | int(dop != 0) << 2 | int(dop == 3) << 3 | int(p.turbulence_correction != 0 or p.motion_correction != 0) << 4 |
                 int(timed) << 5 | int(cols is not None) << 6 | int(cols is not None and cols.inputs_on_device != 0) << 7 |
                 int(method == 'interp_subbeams') << 8 | sum(int(g) << (10 + q) for q, g in enumerate(given)))
        fbits = (int(ray_prep) | int(ray_prep and p.n_hnodes > 1 and p.geometry_mode != BC.HOST_PATHS) << 1 |
                 int(ray_prep and p.geometry_mode == 0 and t.site is None) << 2 | int(dop in (1, 2) and p.n_sub >= MIN_SUB) << 3 |
                 forms['gate1'] << 4 | forms['gate1_ray'] << 5 | forms['rare_direct'] << 6 | forms['subbeam_sum'] << 7)
        row = dict(n_rays=p.n_rays * n_members, ng=p.n_gates, n_sub=p.n_sub, n_h=p.n_hnodes, n_v=p.n_vnodes,
                   n_vars=cols.n_vars if cols is not None else ctx.n_vars, n_hyd=self.n_hyd, n_keys=self.n_keys, n_vb=p.n_vbins,
                   mode=p.geometry_mode, flags=flags, cthreads=256, forms=fbits, g1r=forms['g1r'])
        want = BC.expected(row)
        for name in BC.NAMES:
            b = int(want[name])
            if b and b > self.model[name]:
                self.model[name] = b + b // 8 + 256
        got = ctx.work_buffers()
        assert got == self.model, (self.tag, method, self.calls, {k: (got[k], self.model[k]) for k in got if got[k] != self.model[k]})
        assert ctx.mem_info()[2] == BC.per_gate_literal(ctx.n_vars if ctx.n_vars > 0 else 9, self.n_hyd)
        self.calls += 1
        self.last = row


def conf_sub(n_h, n_v, threshold=1.0):
    conf, luts, cubes, az, el = P.conf_65()
    conf = copy.deepcopy(conf)
    conf['integration'].update(nh_GH=n_h, nv_GH=n_v, weight_threshold=threshold)
    return conf, luts, cubes, az, el


def bit(v, k):
    return (v >> k) & 1


def test_single_beam_grows_and_never_shrinks():
    conf, luts, cubes, az, el = P.conf_65()
    op = E.operator(conf, luts)
    E.load(op, cubes[0])
    w = Watch(op, luts, 'c2_rsg 3 x 65')
    op.simulate_rays(az, el)
    assert (w.last['n_rays'], w.last['ng'], w.last['n_sub']) == (3, 65, 1) and bit(w.last['flags'], 2) == 1
    small = dict(w.model)
    vals = op._ctx.n_vars * 195 * 4
    assert small['vals'] == vals + vals // 8 + 256 and small['gscan'] == 2340 + 292 + 256 and small['defer'] == 195 + 24 + 256
    for absent in ('rayc', 'poly', 'timed', 'coords', 'wgate', 'colin', 'xscr', 'xgeo', 'beam', 'bsigma', 'bon', 'present', 'clk'):
        assert small[absent] == 0, absent
    az7 = az[0] + 0.5 * np.arange(7)
    op.simulate_rays(az7, np.full(7, el[0]))
    big = dict(w.model)
    assert w.last['n_rays'] == 7 and all(big[k] > small[k] for k in ('vals', 'key', 'res', 'vn')) and big['mask'] == small['mask']
    op.simulate_rays(az, el)
    assert w.model == big and w.calls == 3
    op.close()


def test_sub_beams_export_and_columns():
    conf, luts, cubes, az, el = conf_sub(3, 1)
    op = E.operator(conf, luts)
    E.load(op, cubes[0])
    w = Watch(op, luts, 'c2_rsg 3 x 65 x 3')
    op.simulate_rays(az, el)
    assert (w.last['n_rays'], w.last['ng'], w.last['n_sub']) == (3, 65, MIN_SUB - 1) and w.last['forms'] & 15 == 0
    assert w.model['rayc'] == 0 and w.model['poly'] == 0 and w.model['proj'] == 0 and w.model['gscan'] == 0
    op.close()
    conf, luts, cubes, az, el = conf_sub(3, 3, 0.75)
    op = E.operator(conf, luts)
    E.load(op, cubes[0])
    w = Watch(op, luts, 'c2_rsg 3 x 65 x 5')
    op.simulate_rays(az, el)
    assert (w.last['n_rays'], w.last['ng'], w.last['n_h']) == (3, 65, 3) and w.last['n_sub'] == MIN_SUB + 1
    assert bit(w.last['forms'], 0) == 1 and bit(w.last['forms'], 3) == 1          # the per-ray constants, the velocity terms
    for needed in ('rayc', 'poly', 'proj', 'icefirst'):
        assert w.model[needed] > 0, needed
    assert w.model['xscr'] == 0 and w.model['colin'] == 0
    cols = op.interpolate_rays(az, el)
    assert bit(w.last['flags'], 8) == 1 and w.model['xscr'] > 0 and w.model['xgeo'] > 0 and w.model['colin'] == 0
    op.simulate_columns(cols)
    assert bit(w.last['flags'], 6) == 1 and bit(w.last['flags'], 7) == 0 and w.model['colin'] > 0
    assert w.calls == 3
    op.close()


def test_doppler_spectrum_with_broadening():
    import _broadening as B
    import _cases
    from cosmo_pol_amd import RadarOperator
    from cosmo_pol_oracle import config as ocfg
    name = 'd3_turb_motion_sub'
    over, az, el, cube, two = B.case_inputs(name)
    conf = ocfg.make_config(over)
    luts = {h: _cases.synthetic_lut(h, conf['radar']['frequency'], conf['microphysics']['scheme']) for h in ocfg.hydrometeor_list(conf)}
    op = RadarOperator(config=copy.deepcopy(over), luts=luts)
    op.load_model_arrays(cube['data'], cube['zlevels'], cube['proj_info'], cube['resolution'])
    w = Watch(op, luts, name)
    op.simulate_rays([az], [el])
    assert bit(w.last['flags'], 3) == 1 and bit(w.last['flags'], 4) == 1 and w.last['n_sub'] > 1
    for needed in ('beam', 'bsigma', 'bon'):
        assert w.model[needed] > 0, needed
    assert w.model['gscan'] == 0 and w.model['szinteg'] == 0 and w.calls == 1
    op.close()


def test_two_members_and_a_time_blend():
    conf, luts, cubes, az, el = P.conf_65()
    op = E.operator(conf, luts)
    op.load_model_ensemble([c['data'] for c in cubes[:2]], cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
    w = Watch(op, luts, 'two members')
    op.simulate_rays_ensemble(az, el, members=[0, 1], form='shared')
    assert w.last['n_rays'] == 6 and w.model['timed'] == 0 and w.calls == 1
    op.close()
    op = E.operator(conf, luts)
    op.load_model_series([c['data'] for c in cubes], [0.0, 600.0, 1500.0], cubes[0]['zlevels'], cubes[0]['proj_info'], cubes[0]['resolution'])
    w = Watch(op, luts, 'time blend')
    op.simulate_rays_at(az, el, 200.0)
    assert w.last['n_rays'] == 3 and bit(w.last['flags'], 5) == 1
    assert w.model['timed'] == 2 * 3 * 4 + 3 + 256 and w.calls == 1
    op.close()


def test_graph_replay_across_a_regrow(monkeypatch):
    import torch
    conf, luts, cubes, az, el = P.conf_65()
    az7, el7 = az[0] + 0.5 * np.arange(7), np.full(7, el[0])
    fields = ['ZH', 'ZDR', 'KDP', 'RHOHV', 'PHIDP']
    snaps, caps = {}, {}
    for use_graph in ('1', '0'):
        monkeypatch.setenv('CPOL_USE_GRAPH', use_graph)
        op = E.operator(conf, luts, lanes=1)
        E.load(op, cubes[0])
        ctx = op._ctx
        slab = torch.full((len(fields), 7, P.N_GATES), -1.0, dtype=torch.float32, device='cuda')

        def run(azs, els):
            n = len(azs)
            ptrs = {k: slab[i].data_ptr() for i, k in enumerate(fields)}
            op.simulate_rays(azs, els, device_outputs=ptrs)
            ctx.synchronize()
            return slab.cpu().numpy()[:, :n].copy(), ctx.launch_forms(), ctx.work_buffers()

        def captures():
            return int(ctx.debug_read('graph_captures', (1,), np.uint64)[0])
        # the per-gate buffers of seven rays without the single-beam kernel's: the general launch sequence of the debug reads
        ctx.enable_debug(True)
        op.simulate_rays(az7, el7)
        ctx.enable_debug(False)
        held = ctx.work_buffers()
        assert held['gscan'] == 0 and held['defer'] == 0 and held['vals'] > 0
        got = []
        for k in range(3):                                       # A: uploaded, captured into either counter set's graph, replayed
            a, forms, cap_a = run(az, el)
            got.append(a)
            assert forms['gate1'] == 1
            if k:
                assert forms['graph_replayed'] == int(use_graph), (k, forms)
        assert 0 < cap_a['gscan'] < 3 * 7 * P.N_GATES * 4 and cap_a['defer'] >= 7 * P.N_GATES
        b, forms, cap_b = run(az7, el7)                          # B regrows b_gscan and nothing else
        assert forms['gate1'] == 1
        grown = {k for k in cap_b if cap_b[k] != cap_a[k]}
        assert grown == {'gscan'} and 'gscan' not in BC.PARENT_KEY, grown
        before = captures()
        for k in range(2):                                       # A again, on either counter set: captured anew, never replayed over
            a, forms, _ = run(az, el)                            # the graph that holds the replaced b_gscan
            got.append(a)
            assert forms['graph_replayed'] == int(use_graph)
        # (the A on B's counter set always; the other one unless the allocator handed b_gscan its old address back)
        made = captures() - before
        assert (1 <= made <= 2) if use_graph == '1' else made == 0, made
        a, forms, _ = run(az, el)                                # ... and from then on replayed again
        got.append(a)
        assert captures() - before == made
        snaps[use_graph], caps[use_graph] = got, cap_b
        op.close()
    assert caps['1'] == caps['0']
    for k, (x, y) in enumerate(zip(snaps['1'], snaps['0'])):
        assert x.tobytes() == y.tobytes(), k
    for x in snaps['1'][1:]:
        assert x.tobytes() == snaps['1'][0].tobytes()
    assert int(np.isfinite(snaps['1'][0][0]).sum()) > P.N_GATES

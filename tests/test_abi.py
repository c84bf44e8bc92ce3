"""CPU-side checks of the drop-in boundary: the shared library loads without a GPU and
exports exactly the entry points include/mrdis.h declares (no compute calls here)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def mrdis():
    import mrdis as m
    if not os.path.exists(m.LIB_PATH):
        subprocess.check_call(['make', '-C', os.path.dirname(m.LIB_PATH), 'libmrdis_hip.so'])
    return m


def header_symbols():
    txt = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    return sorted(set(re.findall(r'\b(mrdis_[a-z0-9_]+)\s*\(', txt)))


def test_library_exports_every_declared_symbol(mrdis):
    lib = mrdis.hip.load()
    declared = header_symbols()
    assert len(declared) >= 25
    for name in declared:
        assert hasattr(lib, name), f'{name} declared in include/mrdis.h but not exported'
    assert sorted(mrdis.hip.EXPORTED_SYMBOLS) == declared, 'python binding table drifted from the header'


def test_version_and_strerror(mrdis):
    lib = mrdis.hip.load()
    assert lib.mrdis_version() >= 100
    assert lib.mrdis_strerror(0) == b'ok'
    assert lib.mrdis_strerror(-3) == b'workspace too small'


def test_workspace_queries_are_host_only(mrdis):
    lib = mrdis.hip.load()
    assert lib.mrdis_conv2d_bwd_weight_workspace(32, 256, 256, 4, 32, 3, 3, 1, 1) > 0
    assert lib.mrdis_conv2d_bwd_weight_workspace(2, 8, 8, 4, 4, 5, 5, 1, 2) == 0      # 25 taps: unsupported
    assert lib.mrdis_norm_workspace(1, 1 << 20, 64) >= 2 * 64 * 4
    assert lib.mrdis_sumsq_workspace() > 0


def test_missing_library_fails_loudly(mrdis, tmp_path):
    import importlib
    hip = mrdis.hip
    saved = hip._lib
    hip._lib = None
    try:
        with pytest.raises(hip.MrdisLibraryError):
            hip.load(str(tmp_path / 'nope.so'))
    finally:
        hip._lib = saved


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, 'representation-disentanglement_amd')
    for fn in os.listdir(pkg):
        if fn.endswith('.py'):
            src = open(os.path.join(pkg, fn)).read()
            assert 'oracle' not in src.replace('# oracle', ''), fn


def test_mix_job_struct_matches_library():
    """the ctypes mirror of csrc `MixJob` (hip.MixJob) has the library's size; job block counts are positive (host-only calls)"""
    import ctypes
    import mrdis
    lib = mrdis.hip.load()
    assert ctypes.sizeof(mrdis.hip.MixJob) == lib.mrdis_mix_job_bytes() == 368
    assert 1 <= lib.mrdis_mix_job_blocks(32, 16, 9) <= 128


def test_option_and_counter_tables_match_the_library(mrdis):
    """hip.OPTION_NAMES / hip.KERNEL_FAMILIES (what tests/conftest.py snapshots and the parity tests assert on) are names the library knows;
    the dynamic-LDS table hands out whole lines only (host-only calls)."""
    hip = mrdis.hip
    lib = hip.load()
    snap = hip.options_snapshot()
    assert len(snap) == len(hip.OPTION_NAMES) == len(set(hip.OPTION_NAMES))
    for name, v in snap.items():
        hip.set_option(name, v)                    # raises on a name the library does not know
    assert lib.mrdis_set_option(b'no_such_option', 1) == -1
    for fam in hip.KERNEL_FAMILIES + hip.CONV3D_FAMILIES:
        assert lib.mrdis_launch_count(fam.encode()) >= 0, fam
    assert not set(hip.CONV3D_FAMILIES) & set(hip.KERNEL_FAMILIES + hip.VARIANT_FAMILIES + hip.LATENT_FAMILIES)
    assert set(hip.CONV3D_FAMILIES) <= set(hip.launch_counts())
    for fam in hip.ELEM_FAMILIES:          # handed out by launch_counts(elem=True) only
        assert lib.mrdis_launch_count(fam.encode()) >= 0, fam
    assert not set(hip.ELEM_FAMILIES) & set(hip.launch_counts()) and set(hip.ELEM_FAMILIES) <= set(hip.launch_counts(elem=True))
    assert len(set(hip.ELEM_FAMILIES)) == len(hip.ELEM_FAMILIES) == 12
    assert lib.mrdis_launch_count(b'no_such_family') == -1
    assert isinstance(hip.dynamic_lds(), dict)
    import ctypes
    tiny = ctypes.create_string_buffer(4)
    assert lib.mrdis_dynamic_lds_table(tiny, 4) >= 0 and b'=' not in tiny.value.replace(b'\n', b'')[:0]


OPTION_DEFAULTS = {
    'wino': 1, 'nt_mb': 128, 'wino_pipe': 1, 'wino_u': 1, 'wino4': 1, 'wino4r': 1, 'bconv4': 1, 'split6': 1,
    'debug_no16': 0, 'debug_nothin': 0, 'debug_noc4': 0, 'debug_nodma': 0, 'debug_no16_3d': 0, 'debug_bilgen': 0, 'debug_now16': 0, 'debug_nopack': 0,
    'debug_mode': -1, 'debug_bn': -1, 'debug_kc': -1, 'debug_bm': -1, 'debug_c4_tw': -1, 'debug_wgsplit': -1, 'debug_bn3': -1, 'debug_kc3': -1,
    'c4_grid': 0, 'debug_c4_blocks': -1, 'zsearch_grid': 0, 'debug_volgen': 0}


def test_options_read_their_environment_once_at_load(mrdis):
    """one environment variable per option kind, set before a FRESH process loads the library: a value switch with a default (MRDIS_WINO=0), a flag
    (MRDIS_DEBUG_NO16 present, empty = 1) and a value switch that is unset by default (MRDIS_DEBUG_KC=16); every other option reads its default
    (host-only calls, no kernel launch)"""
    import json
    import sys
    assert set(OPTION_DEFAULTS) == set(mrdis.hip.OPTION_NAMES)
    child = ('import ctypes, json, sys\n'
             'lib = ctypes.CDLL(sys.argv[1])\n'
             'lib.mrdis_get_option.restype, lib.mrdis_get_option.argtypes = ctypes.c_longlong, [ctypes.c_char_p]\n'
             'print(json.dumps({n: lib.mrdis_get_option(n.encode()) for n in sys.argv[2:]}))\n')
    env = {k: v for k, v in os.environ.items() if not k.startswith('MRDIS_')}
    env.update(MRDIS_WINO='0', MRDIS_DEBUG_NO16='', MRDIS_DEBUG_KC='16')
    out = subprocess.run([sys.executable, '-c', child, mrdis.LIB_PATH] + list(mrdis.hip.OPTION_NAMES), env=env, check=True,
                         capture_output=True, text=True, timeout=120).stdout
    got = json.loads(out.strip().splitlines()[-1])
    want = dict(OPTION_DEFAULTS, wino=0, debug_no16=1, debug_kc=16)
    assert got == want, {n: (got.get(n), want[n]) for n in want if got.get(n) != want[n]}


def test_library_issues_no_memset_or_memcpy_calls():
    """the training step is recorded into HIP graphs (trainer.GraphedTrainStep): a hipMemsetAsync node did not run again on later replays (round 6, max_pool
    backward), so device buffers are cleared / copied by kernels only"""
    import glob
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'representation-disentanglement_amd', 'csrc')
    bad = []
    for f in sorted(glob.glob(os.path.join(root, '*.hip')) + glob.glob(os.path.join(root, '*.h'))):
        for n, line in enumerate(open(f), 1):
            code = line.split('//')[0]
            if re.search(r'hipMem(set|cpy)\w*\s*\(', code):
                bad.append(f'{os.path.basename(f)}:{n}')
    assert not bad, bad


def test_launch_setup_lives_in_one_place():
    """LDS opt-ins, CU counts and occupancy queries go through mrdis_lds_optin / mrdis_cu_count / mrdis_occupancy (mrdis_runtime.hip), which cache per
    kernel address and are safe from any thread: forward launches run on the main thread, backward ones on autograd's.  No launcher keeps a
    function-local cache of its own (a mutable host static)"""
    import glob
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'representation-disentanglement_amd', 'csrc')
    setup_call = re.compile(r'\b(hipFuncSetAttribute|hipGetDeviceProperties|hipDeviceGetAttribute|hipOccupancyMaxActiveBlocksPerMultiprocessor)\b')
    local_static = re.compile(r'^\s+static\s+(?!(const|constexpr|inline|__device__|__shared__)\b)')
    bad = []
    for f in sorted(glob.glob(os.path.join(root, '*.hip')) + glob.glob(os.path.join(root, '*.h'))):
        if os.path.basename(f) == 'mrdis_runtime.hip':
            continue
        for n, line in enumerate(open(f), 1):
            code = line.split('//')[0]
            if setup_call.search(code) or local_static.search(code):
                bad.append(f'{os.path.basename(f)}:{n}')
    assert not bad, bad


def _file_scope_statements(text):
    """(head, end, scopes) of every file-scope statement of a C++ source, comments / literals / preprocessor lines stripped: head is the text up to its
    ';' (end == ';': a declaration) or up to the '{' of its body (end == '{': a definition, whose body is skipped); scopes names the `extern "C" { }` ('C')
    and namespace ('anon' / 'named') blocks around it, which do not end file scope"""
    import re
    text = re.sub(r'//[^\n]*|/\*.*?\*/|"(?:\\.|[^"\\\n])*"|\'(?:\\.|[^\'\\\n])*\'',
                  lambda m: '"C"' if m.group(0) == '"C"' else ('""' if m.group(0)[0] == '"' else ' '), text, flags=re.S)
    text = re.sub(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', '', text, flags=re.M)
    out, stack, start = [], [], 0              # stack: one entry per open '{': 'body' or a transparent scope
    for i, c in enumerate(text):
        inside = 'body' in stack
        if c == '{':
            head = text[start:i]
            if not inside and re.search(r'\bextern\s+"C"\s*$', head):
                stack.append('C'); start = i + 1
            elif not inside and re.search(r'\bnamespace(\s+\w+)?\s*$', head):
                stack.append('named' if re.search(r'\bnamespace\s+\w+\s*$', head) else 'anon'); start = i + 1
            else:
                if not inside:
                    out.append((head, '{', tuple(stack)))
                stack.append('body')
        elif c == '}':
            if stack:
                stack.pop()
            if 'body' not in stack:
                start = i + 1
        elif c == ';' and not inside:
            out.append((text[start:i], ';', tuple(stack)))
            start = i + 1
    return out


def test_internal_launchers_are_declared_once_in_a_header():
    """a function that crosses a file boundary is declared in ONE header that both its defining file and its callers include (mrdis_launchers.h for the kernel
    launchers; mrdis_common.h includes it), so a parameter list that drifts is a compile or link error (the Makefile links with --no-undefined) and not an
    undefined symbol at dlopen.  No .hip file types a prototype of its own, and every mrdis_* function that a .hip file defines with external linkage (not
    static, not in an anonymous namespace, not extern "C") has exactly one declaration among csrc/*.h and include/mrdis.h"""
    import glob
    import re
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    root = os.path.join(repo, 'representation-disentanglement_amd', 'csrc')
    named = re.compile(r'\s*([^()=]*?)\b(mrdis_\w+)\s*\(')        # `type mrdis_name(`: the name comes before the first parenthesis, a type before the name

    def functions(path):
        for head, end, scopes in _file_scope_statements(open(path).read()):
            m = named.match(head)
            if m and m.group(1).strip():
                yield m.group(2), m.group(1), end, scopes

    prototypes, defined = [], {}
    sources = sorted(glob.glob(os.path.join(root, '*.hip')))
    assert len(sources) >= 32
    for f in sources:
        for name, pre, end, scopes in functions(f):
            if end == ';':
                prototypes.append(f'{os.path.basename(f)}: {name}')
            elif not (re.search(r'\b(static|__device__|__global__)\b|extern\s+"C"', pre) or 'C' in scopes or 'anon' in scopes):
                defined.setdefault(name, os.path.basename(f))
    declared = {}
    for h in sorted(glob.glob(os.path.join(root, '*.h'))) + [os.path.join(repo, 'include', 'mrdis.h')]:
        for name, pre, end, scopes in functions(h):
            if end == ';':
                declared.setdefault(name, []).append(os.path.basename(h))
    assert not prototypes, (len(prototypes), prototypes)
    assert len(defined) >= 50 and 'mrdis_run_wino4' in defined and 'mrdis_opt' in defined, sorted(defined)       # the scan sees the launchers at all
    wrong = {n: (f, declared.get(n, [])) for n, f in defined.items() if len(declared.get(n, [])) != 1}
    assert not wrong, wrong


# ---------------------------------------------------------------- the tables hip.py mirrors by hand, pinned to their sources
def _header_text():
    """include/mrdis.h without comments"""
    txt = open(os.path.join(ROOT, 'include', 'mrdis.h')).read()
    return re.sub(r'/\*.*?\*/|//[^\n]*', ' ', txt, flags=re.S)


def _c_class(decl):
    """pointer | int | long long | size_t | float | double | void of one C parameter or return type (qualifiers and the parameter's name dropped)"""
    decl = re.sub(r'\b(const|unsigned|signed|struct)\b', ' ', decl)
    if '*' in decl or '[' in decl:
        return 'pointer'
    words = decl.split()
    for kind in ('long long', 'size_t', 'double', 'float', 'void', 'int32_t', 'int', 'char'):
        if words[:len(kind.split())] == kind.split():
            return {'int32_t': 'int'}.get(kind, kind)
    raise AssertionError(f'unclassified C type: {decl!r}')


def header_prototypes():
    """{name: (return class, [parameter classes])} of every `type mrdis_name(args);` of include/mrdis.h"""
    txt = re.sub(r'^[ \t]*#(?:[^\n]*\\\n)*[^\n]*', '', _header_text(), flags=re.M)
    out = {}
    for ret, name, args in re.findall(r'([A-Za-z_][\w \t\n\*]*?)\b(mrdis_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', txt):
        params = [] if args.strip() in ('', 'void') else [_c_class(a) for a in args.split(',')]
        assert name not in out, name
        out[name] = (_c_class(ret), params)
    return out


def _ctypes_class(t):
    import ctypes as c
    return {None: 'void', c.c_void_p: 'pointer', c.c_char_p: 'pointer', c.c_int: 'int', c.c_longlong: 'long long', c.c_size_t: 'size_t',
            c.c_float: 'float', c.c_double: 'double'}[t]


def test_signature_table_matches_every_prototype(mrdis):
    """hip._SIGS against the prototypes of include/mrdis.h, position by position: a parameter added to a prototype and not to the table would shift
    every later argument of the call (pointers become integers silently), and the name comparison above does not see it"""
    protos, sigs = header_prototypes(), mrdis.hip._SIGS
    assert len(protos) == len(sigs) and set(protos) == set(sigs), set(protos) ^ set(sigs)      # (the count: a prototype the regex missed cannot hide)
    wrong = {}
    for name, (res, args) in sigs.items():
        got = (_ctypes_class(res), [_ctypes_class(a) for a in args])
        if got != protos[name]:
            wrong[name] = (got, protos[name])
    assert not wrong, wrong


def _x_macro_names(macro):
    """the quoted names of an X-macro table of csrc/mrdis_common.h, in order"""
    txt = open(os.path.join(ROOT, 'representation-disentanglement_amd', 'csrc', 'mrdis_common.h')).read()
    body = re.search(r'#define\s+' + macro + r'\(X\)((?:[^\n]*\\\n)*[^\n]*)', txt).group(1)
    body = re.sub(r'/\*.*?\*/', ' ', body, flags=re.S)
    return re.findall(r'X\(\s*\w+\s*,\s*"([^"]+)"', body)


def test_counter_families_are_the_library_table(mrdis):
    hip = mrdis.hip
    names = _x_macro_names('MRDIS_COUNTERS')
    assert len(names) == len(set(names)) >= 1
    union = sum((v for k, v in sorted(vars(hip).items()) if k.endswith('_FAMILIES') and k != 'KERNEL_FAMILIES'), ())
    assert hip.KERNEL_FAMILIES is hip.WINO_FAMILIES
    assert len(union) == len(set(union)) == len(names) and set(union) == set(names), set(union) ^ set(names)
    assert sorted(hip.launch_counts(elem=True)) == sorted(names)
    assert sorted(hip.launch_counts()) == sorted(set(names) - set(hip.ELEM_FAMILIES))


def test_counter_union_is_built_once(mrdis):
    """the module constants launch_counts() reads instead of summing the family tuples on every call"""
    hip = mrdis.hip
    assert sorted(hip.ALL_COUNTERS) == sorted(_x_macro_names('MRDIS_COUNTERS')) and hip.ALL_COUNTERS == hip.LAUNCH_COUNTERS + hip.ELEM_FAMILIES
    assert tuple(hip.launch_counts(elem=True)) == hip.ALL_COUNTERS and tuple(hip.launch_counts()) == hip.LAUNCH_COUNTERS


def test_option_names_are_the_library_table_in_order(mrdis):
    assert tuple(_x_macro_names('MRDIS_OPTIONS')) == mrdis.hip.OPTION_NAMES


def _int_expr(text):
    """value of a literal integer expression of the header: decimal / hex literals, parentheses, << | + - *; nothing is evaluated as code"""
    toks = re.findall(r'0[xX][0-9a-fA-F]+|\d+|<<|[()|+\-*]', text)
    assert ''.join(toks) == re.sub(r'\s+', '', text), text
    pos = 0

    def atom():
        nonlocal pos
        t = toks[pos]; pos += 1
        if t == '(':
            v = expr(0); assert toks[pos] == ')'; pos += 1
            return v
        if t == '-':
            return -atom()
        return int(t, 0)

    prec = {'|': 1, '<<': 2, '+': 3, '-': 3, '*': 4}

    def expr(level):
        nonlocal pos
        v = atom()
        while pos < len(toks) and toks[pos] in prec and prec[toks[pos]] > level:
            op = toks[pos]; pos += 1
            r = expr(prec[op])
            v = {'|': v | r, '<<': v << r, '+': v + r, '-': v - r, '*': v * r}[op]
        return v

    v = expr(0)
    assert pos == len(toks), text
    return v


def test_mirrored_constants_have_the_header_values(mrdis):
    import torch
    hip = mrdis.hip
    assert _int_expr('(1 << 30)') == 1 << 30 and _int_expr('0x100') == 256 and _int_expr('-2') == -2 and _int_expr('2 + 3 * 4 | 1') == 15
    defs = {m.group(1): _int_expr(m.group(2)) for m in re.finditer(r'^[ \t]*#define[ \t]+MRDIS_(\w+)[ \t]+([^\n]*\S)[ \t]*$', _header_text(), flags=re.M)
            if re.fullmatch(r'[\s0-9a-fA-FxX()<|+\-*]+', m.group(2))}
    mirrors = {n: getattr(hip, n) for n in ('SYNTH_MAX_SRC', 'SEG2D_MAX_SETS', 'SEG2D_MAX_VIEWS', 'FUSE_MAX_SRC', 'EDT_FAR', 'EDT_MAX_SRC', 'SURF_MAX_REGIONS', 'KL_MAXM',
                                            'DT_F32', 'DT_F32_BF16M', 'DT_BF16', 'DT_XBF16_YF32', 'DT_XF32_YBF16', 'DT_DW_PAD16')}
    for tag, dt in (('U8', torch.uint8), ('I16', torch.int16), ('I32', torch.int32), ('F32', torch.float32), ('F64', torch.float64), ('U16', torch.uint16)):
        mirrors['PREP_' + tag] = hip.PREP_DTYPES[dt]
    assert len(hip.PREP_DTYPES) == 6
    for prefix, names in (('PREP_', hip.PREP_KINDS), ('PREP_', hip.PREP_LAYOUTS), ('EXPORT_', hip.EXPORT_KINDS), ('FUSE_', hip.FUSE_METHODS)):
        for i, n in enumerate(names):
            mirrors[prefix + n.upper().replace('-', '_')] = i
    wrong = {n: (v, defs.get(n)) for n, v in mirrors.items() if defs.get(n) != v}
    assert not wrong, wrong


def test_binding_has_no_assert_statement():
    """python -O strips `assert`: a guard of a raw pointer is an `if ...: raise MrdisError`"""
    import ast
    tree = ast.parse(open(os.path.join(ROOT, 'representation-disentanglement_amd', 'hip.py')).read())
    assert not [n.lineno for n in ast.walk(tree) if isinstance(n, ast.Assert)]

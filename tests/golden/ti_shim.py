"""A stand-in for the Taichi vocabulary of the reference's kernels.py / fields.py.

TEST INFRASTRUCTURE ONLY, used by gen_kernel_paths.py when fixtures are
generated (where the reference is present). It is never imported at test time
and never on a GPU machine. load() reads the reference's kernels.py and
fields.py with `ast`, rewrites the tree where plain Python and Taichi differ
(rows marked "rewrite" below) and compiles it in memory: no byte code is
written and nothing of the reference is copied. The reference's own text then
runs on the CPU, serially, in f32.

Two things are not Taichi's but the project's contract, so that the result is
comparable bit for bit with oracle/pt_oracle.c: `ti.random()` is the n-th value
of the current path's counter-based stream (include/ptmi_rng.h, taken from
oracle.rng_probe, never restated here) and the six transcendentals are
include/ptmi_math.h's (oracle.math_probe).

SEMANTICS is the whole surface that still rests on review: one row per Taichi
construct emulated: (construct, semantics chosen, what it serves). SWITCHES
lists the rows that can be flipped for the generator's negative controls.
Both are plain literals: tests/test_kernel_paths.py reads them with
ast.literal_eval, without importing this module.
"""
import ast
import itertools
import os
import sys
import types

import numpy as np

SEMANTICS = [
    ('f32 scalar', 'numpy.float32: + - * / and sqrt correctly rounded, one rounding per operation, no '
     'contraction', 'include/ptmi_math.h contract; all of kernels.py'),
    ('i32 scalar', 'numpy.int32 (Python int for literals and loop indices); + - * wrap to 32 bits',
     'kernels.py:120-138, 970'),
    ('i32 op f32', 'rewrite: every binary operator goes through binop(): the i32 side is cast to f32, the '
     'result is f32; a Python float or float64 operand raises', 'kernels.py:189-190 (px + offset_x)'),
    ('float literal', 'rewrite: every float literal, and math.pi, becomes an f32 value where it is written '
     '(2.0 * math.pi: f32(2) * f32(pi) = f32(2 pi) exactly)', 'kernels.py:52, 97-100; Q21 1e10, Q15 1e8'),
    ('vec3 + - * /', 'immutable; componentwise, a scalar operand is broadcast (cast to f32 first)',
     'kernels.py:71, 188-190, 245-246'),
    ('vec3.dot', '(x*x\' + y*y\') + z*z\', left to right', 'include/ptmi_math.h pt_dot'),
    ('vec3.cross', '(ay*bz - az*by, az*bx - ax*bz, ax*by - ay*bx)', 'kernels.py:67-68, 267, 285, 345-346'),
    ('vec3.norm / normalized', 'norm = sqrt(dot); normalized = v * (1 / sqrt(dot))', 'Q31'),
    ('ti.math.vec3(a)', 'one argument broadcasts to the three components', 'kernels.py:19, 1038'),
    ('and / or', 'rewrite: both operands are evaluated, then combined (Taichi\'s default '
     'short_circuit_operators=False)', 'Q28, kernels.py:894'),
    ('// and %', 'on i32: floor division and floor modulo (Python semantics)', 'Q9, kernels.py:970, 1278-1279'),
    ('a if c else b', 'Python\'s lazy evaluation: both sides are pure in every use (kernels.py:479-481, '
     '509, 643-645, 884-885, 1258), so it equals Taichi\'s select', 'Q15'),
    ('if / a if c else b', 'rewrite: the test passes through br(line, value), which counts the outcome per '
     'path and returns it unchanged', 'coverage_* counters'),
    ('x += v', 'rewrite: x = binop(+, x, v); on a field element, field.aug(index, +, v)',
     'kernels.py:129-149, 1187, 1280, 1373'),
    ('ti.atomic_add(f[i], v)', 'rewrite: adds to the field element and returns the old value',
     'kernels.py:1345, 1375, 1394'),
    ('ti.field / ti.Vector.field', 'numpy array per field; [i], [i, j], [None]; a store casts to the '
     'field\'s type (float64 camera values round to f32 once); from_numpy / to_numpy', 'fields.py:25-277'),
    ('@ti.dataclass .field', 'one numpy array per member; node = f[i] reads and writes through',
     'fields.py:52-62, renderer.py:218-226'),
    ('struct-for, ti.ndrange, range', 'serial loops in index order (row-major)', 'kernels.py:1184, 1225, 1248'),
    ('kernel loop hook', 'rewrite: the first statement of every top-level loop of a @ti.kernel calls '
     'hook(kernel, loop variables); the generator uses it to name the running path', 'ti.random stream'),
    ('ti.Vector([..], dt=ti.i32)', 'mutable list of i32', 'kernels.py:649'),
    ('@ti.func / @ti.kernel / ti.static', 'identity', 'kernels.py'),
    ('ti.cast(x, ti.i32)', 'truncation toward zero; NaN -> 0, saturating (include/ptmi_math.h pt_f2i)',
     'kernels.py:120-122, 970, 995-996'),
    ('ti.cast(x, ti.f32)', 'int -> f32, round to nearest', 'kernels.py:142-148, 995-996, 1153'),
    ('ti.sqrt / ti.abs / ti.floor', 'numpy on f32 (exact)', 'kernels.py'),
    ('ti.min / ti.max', 'IEEE minNum / maxNum on f32 (numpy fmin / fmax), componentwise on vec3, integer '
     'min / max on i32', 'kernels.py:614-619, 991-1000, 1148'),
    ('ti.sin / cos / log / acos / atan2', 'include/ptmi_math.h through oracle.math_probe', 'kernels.py:54-55, 96-97, 441, 1013'),
    ('ti.pow(x, 5.0)', 'include/ptmi_math.h pt_pow5f through oracle.math_probe; any other exponent raises',
     'kernels.py:786'),
    ('ti.random()', 'next value of the current path\'s stream pt_rand(pt_path_key(seed, pixel, sample), n) '
     'through oracle.rng_probe; draws are counted per path', 'include/ptmi_rng.h'),
    ('any other ti.* name', 'raises ShimError; nothing falls back to float64', ''),
]

# name -> the SEMANTICS row it flips. 'control': the generator stores the
# rerun's colours as control_<name> and requires >= 5 differing paths.
# c_mod cannot be a control: kernels.py applies % only to `... % 2 == 0`
# (:970: -1 and 1 are both != 0) and to the non-negative pixel index (:1278-1279,
# with //), so floor and truncated modulo give the same image by construction;
# the generator asserts exactly that and stores the rerun as invariant_c_mod.
SWITCHES = {
    'short_circuit_or': {'row': 'and / or', 'control': True},
    'normalized_div': {'row': 'vec3.norm / normalized', 'control': True},
    'literals_f64': {'row': 'float literal', 'control': True},
    'c_mod': {'row': '// and %', 'control': False},
}

F32, I32 = np.float32, np.int32
CFG = {k: False for k in SWITCHES}


class ShimError(Exception):
    pass


# ---------------------------------------------------------------- scalars
def _is_int(x):
    return isinstance(x, (int, I32)) and not isinstance(x, (bool, np.bool_))


def _to_f(x):
    """Taichi's implicit cast of an operand that meets an f32."""
    if isinstance(x, F32):
        return x
    if _is_int(x):
        return F32(x)
    if isinstance(x, (float, np.float64)):
        if CFG['literals_f64']:
            return np.float64(x)
        raise ShimError('a float64 value reached f32 arithmetic')
    raise ShimError(f'not a scalar: {type(x).__name__}')


def _wrap(v):
    return I32((int(v) + 0x80000000) % 0x100000000 - 0x80000000)


def _int_binop(op, a, b):
    a, b = int(a), int(b)
    if op in ('//', '%'):
        if b == 0:
            raise ShimError('integer division by zero')
        if CFG['c_mod']:
            q = abs(a) // abs(b) * (1 if (a < 0) == (b < 0) else -1)
            return _wrap(q if op == '//' else a - q * b)
        return _wrap(a // b if op == '//' else a % b)
    if op == '+':
        return _wrap(a + b)
    if op == '-':
        return _wrap(a - b)
    if op == '*':
        return _wrap(a * b)
    if op == '&':
        return _wrap(a & b)
    if op == '^':
        return _wrap(a ^ b)
    if op == '|':
        return _wrap(a | b)
    raise ShimError(f'i32 {op} i32 is not in the table')


def _f_binop(op, a, b):
    if op == '+':
        return a + b
    if op == '-':
        return a - b
    if op == '*':
        return a * b
    if op == '/':
        return a / b
    raise ShimError(f'f32 {op} f32 is not in the table')


def binop(op, a, b):
    if isinstance(a, vec) or isinstance(b, vec):
        n = len(a.c) if isinstance(a, vec) else len(b.c)
        ac = a.c if isinstance(a, vec) else (_to_f(a),) * n
        bc = b.c if isinstance(b, vec) else (_to_f(b),) * n
        if len(ac) != len(bc):
            raise ShimError('vector length mismatch')
        return vec(_f_binop(op, x, y) for x, y in zip(ac, bc))
    if _is_int(a) and _is_int(b):
        return _int_binop(op, a, b)
    return _f_binop(op, _to_f(a), _to_f(b))


class vec:
    """Immutable f32 vector (vec3; also the vec4 of fields.sphere_data)."""
    __slots__ = ('c',)

    def __init__(self, comps):
        object.__setattr__(self, 'c', tuple(x if isinstance(x, F32) else F32(x) for x in comps))

    def __setattr__(self, k, v):
        raise ShimError('vec3 is immutable')

    x = property(lambda s: s.c[0])
    y = property(lambda s: s.c[1])
    z = property(lambda s: s.c[2])

    def __getitem__(self, i):
        return self.c[int(i)]

    def __len__(self):
        return len(self.c)

    def __neg__(self):
        return vec(-x for x in self.c)

    def dot(self, o):
        r = self.c[0] * o.c[0]
        for a, b in zip(self.c[1:], o.c[1:]):
            r = r + a * b
        return r

    def cross(self, o):
        a, b = self.c, o.c
        return vec((a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]))

    def norm(self):
        return np.sqrt(self.dot(self))

    def normalized(self):
        if CFG['normalized_div']:
            n = self.norm()
            return vec(x / n for x in self.c)
        inv = F32(1.0) / np.sqrt(self.dot(self))
        return vec(x * inv for x in self.c)


def _vec3(*a):
    if len(a) == 1:
        a = a * 3
    if len(a) != 3:
        raise ShimError('vec3 takes 1 or 3 components')
    return vec(F32(_to_f(x)) for x in a)


# ---------------------------------------------------------------- fields
class Field:
    def __init__(self, n, dtype, shape):
        shape = () if shape is None else ((int(shape),) if np.isscalar(shape) else tuple(int(s) for s in shape))
        self.n, self.shape = n, shape
        self.arr = np.zeros(shape + ((n,) if n else ()), np.float32 if dtype is f32 else np.int32)

    def _ix(self, i):
        if i is None:
            return ()
        return tuple(int(k) for k in i) if isinstance(i, tuple) else (int(i),)

    def __getitem__(self, i):
        v = self.arr[self._ix(i)]
        if self.n:
            return vec(v) if self.arr.dtype == np.float32 else tuple(I32(x) for x in v)
        return self.arr.dtype.type(v)

    def __setitem__(self, i, v):
        self.arr[self._ix(i)] = v.c if isinstance(v, vec) else v

    def aug(self, i, op, v):
        self[i] = binop(op, self[i], v)

    def atomic_add(self, i, v):
        old = self[i]
        self[i] = binop('+', old, v)
        return old

    def from_numpy(self, a):
        self.arr[...] = a

    def to_numpy(self):
        return self.arr.copy()

    def __iter__(self):
        for ix in np.ndindex(*self.shape):
            yield ix if len(ix) > 1 else ix[0]


class _StructRef:
    def __init__(self, sf, i):
        object.__setattr__(self, '_sf', sf)
        object.__setattr__(self, '_i', int(i))

    def __getattr__(self, k):
        return self._sf.members[k][self._i]

    def __setattr__(self, k, v):
        self._sf.members[k][self._i] = v


class _StructField:
    def __init__(self, ann, shape):
        self.members = {}
        for k, t in ann.items():
            if t is _vec3:
                self.members[k] = Field(3, f32, shape)
            elif t is f32 or t is i32:
                self.members[k] = Field(0, t, shape)
            else:
                raise ShimError(f'struct member type of {k} is not in the table')

    def __getitem__(self, i):
        return _StructRef(self, i)


class _StructType:
    def __init__(self, cls):
        self.ann = dict(cls.__annotations__)

    def field(self, shape):
        return _StructField(self.ann, shape)


class _IVec:
    def __init__(self, vals):
        self.v = [I32(x) for x in vals]

    def __getitem__(self, i):
        return self.v[int(i)]

    def __setitem__(self, i, x):
        if not _is_int(x):
            raise ShimError('i32 vector element')
        self.v[int(i)] = I32(x)


class _VectorNS:
    def __call__(self, vals, dt=None):
        if dt is not i32:
            raise ShimError('ti.Vector(..., dt) other than i32 is not in the table')
        return _IVec(vals)

    @staticmethod
    def field(n, dtype, shape=None):
        return Field(int(n), dtype, shape)


class _Type:
    def __init__(self, name):
        self.name = name


f32, i32 = _Type('f32'), _Type('i32')


# ---------------------------------------------------------------- the streams
class PathStreams:
    """ti.random(): per-path counters over oracle.rng_probe's stream."""

    def __init__(self, rng_probe, seed):
        self.probe, self.seed = rng_probe, int(seed)
        self.cur = None
        self.count, self.buf = {}, {}

    def set_path(self, pixel, sample):
        self.cur = (int(pixel), int(sample))

    def draws(self, pixel, sample):
        return self.count.get((int(pixel), int(sample)), 0)

    def draw(self):
        if self.cur is None:
            raise ShimError('ti.random() outside a path')
        n = self.count.get(self.cur, 0)
        b = self.buf.get(self.cur)
        if b is None or n >= len(b):
            b = self.buf[self.cur] = self.probe(self.seed, self.cur[0], self.cur[1], max(64, 4 * n))[0]
        self.count[self.cur] = n + 1
        return F32(b[n])


class State:
    def __init__(self, streams, math_probe):
        self.streams, self.math_probe = streams, math_probe
        self.hook = None          # hook(kernel name, {loop variable: value})
        self.events = None        # set of (file, line, outcome...) of the running path
        self.branch = {}          # (file, line, outcome...) -> count


def _make_ti(st):
    def m1(fn):
        def f(x):
            return F32(st.math_probe(fn, np.array([_to_f(x)], np.float32))[0])
        return f

    def atan2(y, x):
        return F32(st.math_probe('atan2', np.array([_to_f(y)], np.float32), np.array([_to_f(x)], np.float32))[0])

    def pow_(x, e):
        if not (isinstance(e, (F32, np.float64)) and float(e) == 5.0):
            raise ShimError('ti.pow exponent other than 5.0 is not in the table')
        return F32(st.math_probe('pow5', np.array([_to_f(x)], np.float32))[0])

    def minmax(ff, fi):
        def f(a, b):
            if isinstance(a, vec) and isinstance(b, vec):
                return vec(ff(x, y) for x, y in zip(a.c, b.c))
            if _is_int(a) and _is_int(b):
                return I32(fi(int(a), int(b)))
            return ff(_to_f(a), _to_f(b))
        return f

    def cast(x, t):
        if t is i32:
            if _is_int(x):
                return I32(x)
            x = _to_f(x)
            if x != x:
                return I32(0)
            if x >= 2147483648.0:
                return I32(2147483647)
            if x <= -2147483648.0:
                return I32(-2147483648)
            return I32(int(x))
        if t is f32:
            return F32(_to_f(x))
        raise ShimError('ti.cast target is not in the table')

    def abs_(x):
        return I32(abs(int(x))) if _is_int(x) else np.abs(_to_f(x))

    def atomic_add(*a):
        raise ShimError('ti.atomic_add on something that is not a field element')

    ident = lambda x=None, **kw: x
    names = {
        'f32': f32, 'i32': i32, 'func': ident, 'kernel': ident, 'static': ident, 'init': lambda **kw: None,
        'sync': lambda: None, 'metal': 'metal', 'dataclass': _StructType,
        'math': types.SimpleNamespace(vec3=_vec3), 'Vector': _VectorNS(),
        'field': lambda dtype, shape=None: Field(0, dtype, shape),
        'ndrange': lambda *n: itertools.product(*(range(int(k)) for k in n)),
        'random': lambda: st.streams.draw(),
        'sqrt': lambda x: np.sqrt(_to_f(x)), 'floor': lambda x: np.floor(_to_f(x)), 'abs': abs_,
        'min': minmax(np.fmin, min), 'max': minmax(np.fmax, max), 'cast': cast,
        'sin': m1('sin'), 'cos': m1('cos'), 'log': m1('log'), 'acos': m1('acos'), 'atan2': atan2, 'pow': pow_,
        'atomic_add': atomic_add,
    }

    class Ti(types.ModuleType):
        def __getattr__(self, k):
            raise ShimError(f'ti.{k} is not in the shim\'s table')

    ti = Ti('taichi')
    ti.__dict__.update(names)
    return ti


# ---------------------------------------------------------------- the loader
_OPS = {ast.Add: '+', ast.Sub: '-', ast.Mult: '*', ast.Div: '/', ast.FloorDiv: '//', ast.Mod: '%',
        ast.BitAnd: '&', ast.BitXor: '^', ast.BitOr: '|'}


def _call(name, *args):
    return ast.Call(ast.Name(name, ast.Load()), list(args), [])


class _Rewrite(ast.NodeTransformer):
    def __init__(self, fname):
        self.fname = fname

    def visit_Constant(self, node):
        if isinstance(node.value, float):
            return _call('_shim_F', node)
        return node

    def visit_Attribute(self, node):
        self.generic_visit(node)
        if isinstance(node.value, ast.Name) and node.value.id == 'math' and node.attr == 'pi':
            return _call('_shim_F', node)
        return node

    def _op(self, op):
        if type(op) not in _OPS:
            raise ShimError(f'operator {type(op).__name__} is not in the table')
        return ast.Constant(_OPS[type(op)])

    def visit_BinOp(self, node):
        self.generic_visit(node)
        return _call('_shim_binop', self._op(node.op), node.left, node.right)

    def visit_AugAssign(self, node):
        self.generic_visit(node)
        t = node.target
        if isinstance(t, ast.Name):
            return ast.Assign([t], _call('_shim_binop', self._op(node.op), ast.Name(t.id, ast.Load()), node.value))
        if isinstance(t, ast.Subscript):
            return ast.Expr(_call('_shim_aug', t.value, t.slice, self._op(node.op), node.value))
        raise ShimError('augmented assignment target is not in the table')

    def visit_BoolOp(self, node):
        self.generic_visit(node)
        if isinstance(node.op, ast.Or) and CFG['short_circuit_or']:
            return node
        return _call('_shim_boolop', ast.Constant('or' if isinstance(node.op, ast.Or) else 'and'),
                     ast.Constant(node.lineno), *node.values)

    def visit_If(self, node):
        self.generic_visit(node)
        node.test = _call('_shim_br', ast.Constant(node.lineno), node.test)
        return node

    visit_IfExp = visit_If

    def visit_Call(self, node):
        self.generic_visit(node)
        f = node.func
        if (isinstance(f, ast.Attribute) and f.attr == 'atomic_add' and isinstance(f.value, ast.Name)
                and f.value.id == 'ti' and isinstance(node.args[0], ast.Subscript)):
            s = node.args[0]
            return _call('_shim_atomic_add', s.value, s.slice, node.args[1])
        return node

    def visit_FunctionDef(self, node):
        self.generic_visit(node)
        is_kernel = any(isinstance(d, ast.Attribute) and d.attr == 'kernel' for d in node.decorator_list)
        if is_kernel:
            for s in node.body:
                if isinstance(s, ast.For):
                    t = s.target
                    names = [t.id] if isinstance(t, ast.Name) else [e.id for e in t.elts]
                    d = ast.Dict([ast.Constant(n) for n in names], [ast.Name(n, ast.Load()) for n in names])
                    s.body.insert(0, ast.Expr(_call('_shim_hook', ast.Constant(node.name), d)))
        return node


class Loaded:
    pass


def load(ref_taichi_dir, switches, rng_probe, math_probe, seed):
    """Compile the reference's fields.py and kernels.py over the shim.
    switches: names of SWITCHES to flip. Returns an object with .ti, .fields,
    .kernels, .state (State) and .package (the stub package they live in)."""
    sys.dont_write_bytecode = True
    np.seterr(all='ignore')
    for k in CFG:
        CFG[k] = k in switches
    unknown = set(switches) - set(CFG)
    if unknown:
        raise ShimError(f'unknown switches {unknown}')
    st = State(PathStreams(rng_probe, seed), math_probe)
    ti = _make_ti(st)
    sys.modules['taichi'] = ti
    pkg_name = 'render_server.taichi_renderer'
    pkg = sys.modules.get(pkg_name)
    if pkg is None:
        raise ShimError('install the package stubs first (gen_fixtures._install_stubs)')

    def boolop(kind, line, *vals):
        t = tuple(bool(v) for v in vals)
        _count(st, (line,) + t)
        return any(t) if kind == 'or' else all(t)

    def br(line, v):
        v = bool(v)
        _count(st, (line, v))
        return v

    def hook(name, variables):
        if st.hook is not None:
            st.hook(name, variables)

    helpers = {'_shim_F': np.float64 if CFG['literals_f64'] else np.float32, '_shim_binop': binop,
               '_shim_aug': lambda f, i, op, v: f.aug(i, op, v), '_shim_boolop': None, '_shim_br': None,
               '_shim_hook': hook, '_shim_atomic_add': lambda f, i, v: f.atomic_add(i, v)}

    out = Loaded()
    for name in ('fields', 'kernels'):
        path = os.path.join(ref_taichi_dir, name + '.py')
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        tree = ast.fix_missing_locations(_Rewrite(name).visit(tree))
        mod = types.ModuleType(f'{pkg_name}.{name}')
        mod.__package__ = pkg_name
        mod.__file__ = path
        mod.__dict__.update(helpers)
        mod.__dict__['_shim_boolop'] = lambda kind, line, *v, _n=name: boolop(kind, (_n, line), *v)
        mod.__dict__['_shim_br'] = lambda line, v, _n=name: br((_n, line), v)
        sys.modules[mod.__name__] = mod
        setattr(pkg, name, mod)
        exec(compile(tree, path, 'exec'), mod.__dict__)
        setattr(out, name, mod)
    out.ti, out.state, out.package = ti, st, pkg
    return out


def _count(st, key):
    st.branch[key] = st.branch.get(key, 0) + 1
    if st.events is not None:
        st.events.add(key)

"""Reader of include/lime_hip.h: the C ABI as ctypes signatures, Structure classes and integer constants.

The header is the checked statement of the ABI (every unit that defines a lime_* entry compiles against it), so the binding is derived
from it instead of written out a second time.  Plain `re` over the subset of C the header uses; a declaration outside that subset
raises ValueError naming the line it starts on -- nothing is skipped.
"""
import ctypes
import re
from ctypes import POINTER, c_char, c_char_p, c_float, c_int32, c_int64, c_uint32, c_uint64, c_void_p

SCALARS = {'int': c_int32, 'int32_t': c_int32, 'int64_t': c_int64, 'uint32_t': c_uint32, 'uint64_t': c_uint64, 'float': c_float,
           'char': c_char}
_DECLARATOR = re.compile(r'^(.*[\s*])(\w+)\s*((?:\[\s*\w+\s*\]\s*)*)$', re.S)


class Header:
    """signatures: name -> (restype, [argtypes]); c_types: name -> (return type, [parameter types]) as the header spells them;
    structs: C name -> ctypes.Structure subclass; constants: enumerator / integer #define -> value."""

    def __init__(self, text, where='lime_hip.h'):
        self.where, self.signatures, self.c_types, self.structs, self.constants = where, {}, {}, {}, {}
        for line, decl in self._declarations(self._preprocess(text)):
            self._line = line
            m = re.match(r'^typedef\s+struct\s*\w*\s*\{(.*)\}\s*(\w+)$', decl, re.S)
            if m:
                self.structs[m.group(2)] = type(m.group(2), (ctypes.Structure,), {'_fields_': self._fields(m.group(1))})
                continue
            m = re.match(r'^(?:typedef\s+)?enum\s*\{(.*)\}\s*\w*$', decl, re.S)
            if m:
                self._enumerators(m.group(1))
                continue
            m = re.match(r'^([\w\s*]*[\s*])(\w+)\s*\(([^(){}]*)\)$', decl, re.S)
            if not m:
                self._fail('cannot read the declaration %r' % ' '.join(decl.split())[:80])
            params = [] if m.group(3).strip() == 'void' else [self._split(p, 'parameter') for p in m.group(3).split(',')]
            if any(bound for _, _, bound in params):
                self._fail('array parameters are not read')
            ret = ' '.join(m.group(1).split())
            self.signatures[m.group(2)] = (self._ctype(ret, None), [self._ctype(t, n) for t, n, _ in params])
            self.c_types[m.group(2)] = (ret, [t for t, _, _ in params])

    def _fail(self, what):
        raise ValueError('%s:%d: %s' % (self.where, self._line, what))

    def _preprocess(self, text):
        """Comments blanked (line numbers kept), integer #defines taken, the C++ branch of `#ifdef __cplusplus` dropped."""
        text = re.sub(r'/\*.*?\*/|//[^\n]*', lambda m: '\n' * m.group(0).count('\n'), text, flags=re.S)
        out, live = [], [True]
        for n, raw in enumerate(text.split('\n'), 1):
            self._line, s = n, raw.strip()
            if not s.startswith('#'):
                out.append(raw if all(live) else '')
                continue
            out.append('')
            word, _, rest = s[1:].strip().partition(' ')
            if word in ('ifdef', 'ifndef'):
                if word == 'ifdef' and rest.strip() != '__cplusplus':
                    self._fail('cannot evaluate #ifdef %s' % rest)
                live.append(word == 'ifndef')           # an include guard is open, __cplusplus is not defined
            elif word == 'else':
                live[-1] = not live[-1]
            elif word == 'endif':
                live.pop()
            elif word == 'define' and all(live) and len(rest.split()) > 1:
                name, value = rest.split(None, 1)
                self.constants[name] = self._int(value)
            elif word not in ('define', 'include'):
                self._fail('cannot read the preprocessor line %r' % s)
        return '\n'.join(out)

    def _declarations(self, text):
        """(first line, text) of every top-level declaration: the text up to a `;` outside braces."""
        depth, start, line = 0, 0, 1
        for m in re.finditer(r'[{};]', text):
            depth += {'{': 1, '}': -1, ';': 0}[m.group(0)]
            if m.group(0) == ';' and depth == 0:
                decl = text[start:m.start()].lstrip()
                line += text.count('\n', start, m.start() - len(decl))
                if decl:
                    yield line, decl.rstrip()
                line += decl.count('\n')
                start = m.end()
        rest = text[start:].lstrip()
        if rest:
            self._line = line + text.count('\n', start, len(text) - len(rest))
            self._fail('unterminated declaration %r' % ' '.join(rest.split())[:80])

    def _int(self, value):
        value = value.strip()
        if value in self.constants:
            return self.constants[value]
        try:
            return int(value, 0)
        except ValueError:
            self._fail('%r is not an integer constant' % value)

    def _enumerators(self, body):
        value = -1
        for item in filter(None, (e.strip() for e in body.split(','))):
            name, eq, v = (s.strip() for s in item.partition('='))
            if not re.match(r'^[A-Za-z_]\w*$', name):
                self._fail('cannot read the enumerator %r' % item)
            value = self._int(v) if eq else value + 1
            self.constants[name] = value

    def _split(self, text, what):
        """'const float* a[3]' -> ('const float*', 'a', ['3']); 'char n[2][64]' -> ('char', 'n', ['2', '64'])"""
        m = _DECLARATOR.match(text.strip())
        if not m or not m.group(1).strip():
            self._fail('cannot read the %s %r' % (what, text))
        return ' '.join(m.group(1).split()), m.group(2), re.findall(r'\w+', m.group(3))

    def _fields(self, body):
        fields = []
        for member in filter(None, (s.strip() for s in body.split(';'))):
            first, *more = member.split(',')
            ctype, name, bounds = self._split(first, 'field')
            base = ctype.split('*')[0]                  # `const float* a, b`: b is a float
            for ctype, name, bounds in [(ctype, name, bounds)] + [self._split(base + ' ' + d, 'field') for d in more]:
                t = self._ctype(ctype, name)
                for bound in reversed(bounds):          # `char n[2][64]`: two arrays of 64
                    t = t * self._int(bound)
                fields.append((name, t))
        return fields

    def _ctype(self, ctype, name):
        base = ' '.join(w for w in ctype.replace('*', ' ').split() if w != 'const')
        stars = ctype.count('*')
        if stars == 0 and base in SCALARS:
            return SCALARS[base]
        if stars == 1 and base == 'char':
            return c_char_p
        if stars == 1 and base in self.structs:
            return POINTER(self.structs[base])
        if stars >= 1 and re.match(r'^\w+$', base):
            return c_void_p
        self._fail('no ctypes class for %r%s' % (ctype, ' (%s)' % name if name else ''))

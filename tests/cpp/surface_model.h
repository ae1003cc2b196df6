// surface_model.h -- the generator and the host model of the SMArray surface fuzzer (tests/cpp/fuzz_surface.cpp runs the programs
// through include/sm.h on the GPU, tests/cpp/surface_model_host.cpp runs them here alone).  No sm.h, no library: plain C++.
//
// A CASE is a list of statements over a pool of named arrays v0 .. v11, drawn from (seed, case) alone.  The generator is steered
// by the model and by nothing else, so the program of a seed is the same with and without a device.  The model is deliberately
// trivial: one dense std::vector<T> per storage, a pool entry is (storage, offset, shape, strides) -- aliasing holds by
// construction --, arithmetic is done in T (integers in the unsigned type: they wrap), an assignment evaluates its right-hand
// side completely and then stores it (numpy's meaning), integer division is csrc/ops.hip.h's: truncation, x / 0 = 0,
// INT_MIN / -1 = INT_MIN.  Build with -ffp-contract=off.
//
// Case::next() draws the next statement, applies it to the model and leaves in the statement what a run must observe (element
// reads, sums, family results); after a COMPARE statement the executor compares its whole pool with Case::model.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <ostream>
#include <sstream>
#include <string>
#include <type_traits>
#include <vector>

namespace sfm {

using Shape = std::vector<std::size_t>;

inline std::size_t prod(const Shape &s) {
    std::size_t n = 1;
    for (std::size_t d : s) n *= d;
    return n;
}
inline Shape dense_strides(const Shape &s) {
    Shape st(s.size());
    std::size_t acc = 1;
    for (std::size_t i = s.size(); i-- > 0;) st[i] = acc, acc *= s[i];
    return st;
}

// splitmix64: the draws depend on (seed, case) alone
struct Rng {
    std::uint64_t s;
    std::uint64_t next() {
        std::uint64_t z = (s += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
    }
    std::size_t below(std::size_t n) { return n ? static_cast<std::size_t>(next() % n) : 0; }
    std::size_t range(std::size_t lo, std::size_t hi) { return lo + below(hi - lo + 1); }  // inclusive
    bool chance(unsigned num, unsigned den) { return below(den) < num; }
};
inline std::uint64_t case_seed(std::uint64_t seed, std::uint64_t k) {
    Rng r{seed * 0x100000001b3ull + 0x51ed27ull};
    r.s ^= r.next() + k * 0xd6e8feb86659fd93ull;
    return r.next();
}

enum SizeClass { TINY = 0, SMALL = 1, MID = 2 };
inline const char *class_name(int c) { return c == TINY ? "tiny" : c == SMALL ? "small" : "mid"; }
// the element type and size class of case k: the types take turns; of 40 cases six are mid (every type within 40), a third of the
// others small, the rest tiny
inline int type_of_case(std::uint64_t k) { return static_cast<int>(k % 4); }
inline int class_of_case(std::uint64_t k) {
    const int j = static_cast<int>(k % 40);
    if (j == 6 || j == 13 || j == 19 || j == 24 || j == 30 || j == 37) return MID;
    return j % 3 == 1 ? SMALL : TINY;
}
template <typename T> struct type_info_of;
template <> struct type_info_of<float> { static constexpr int id = 0; static constexpr const char *name = "float"; };
template <> struct type_info_of<double> { static constexpr int id = 1; static constexpr const char *name = "double"; };
template <> struct type_info_of<int> { static constexpr int id = 2; static constexpr const char *name = "int"; };
template <> struct type_info_of<std::int64_t> { static constexpr int id = 3; static constexpr const char *name = "std::int64_t"; };

// ---- arithmetic in T
template <typename T, bool Float = std::is_floating_point_v<T>> struct Ar;
template <typename T> struct Ar<T, false> {
    using U = std::make_unsigned_t<T>;
    static T add(T a, T b) { return static_cast<T>(static_cast<U>(static_cast<U>(a) + static_cast<U>(b))); }
    static T sub(T a, T b) { return static_cast<T>(static_cast<U>(static_cast<U>(a) - static_cast<U>(b))); }
    static T mul(T a, T b) { return static_cast<T>(static_cast<U>(static_cast<U>(a) * static_cast<U>(b))); }
    static T neg(T a) { return static_cast<T>(static_cast<U>(U{0} - static_cast<U>(a))); }
    static T div(T a, T b) {
        if (b == 0) return 0;
        if (b == -1) return neg(a);
        return a / b;
    }
    static T abs(T a) { return a < 0 ? neg(a) : a; }
    static T sqrtabs(T a) { return a; }  // not drawn for integers
    static T ipow(T a, int k) {
        U r = 1;
        for (int i = 0; i < k; ++i) r = static_cast<U>(r * static_cast<U>(a));
        return static_cast<T>(r);
    }
};
template <typename T> struct Ar<T, true> {
    static T add(T a, T b) { return a + b; }
    static T sub(T a, T b) { return a - b; }
    static T mul(T a, T b) { return a * b; }
    static T div(T a, T b) { return a / b; }
    static T neg(T a) { return -a; }
    static T abs(T a) { return std::fabs(a); }
    static T sqrtabs(T a) { return std::sqrt(std::fabs(a)); }
    static T ipow(T a, int) { return a; }  // not drawn for floats
};
template <typename T> T arith(int op, T a, T b) {
    switch (op) {
        case 0: return Ar<T>::add(a, b);
        case 1: return Ar<T>::sub(a, b);
        case 2: return Ar<T>::mul(a, b);
        default: return Ar<T>::div(a, b);
    }
}
template <typename T> bool is_nan(T v) {
    if constexpr (std::is_floating_point_v<T>) return v != v;
    else return false;
}
template <typename T> bool is_finite(T v) {
    if constexpr (std::is_floating_point_v<T>) return std::isfinite(v);
    else return true;
}
// bit for bit, except that a NaN on both sides counts as equal (the sign of a generated NaN differs between x86 and the GPU)
template <typename T> bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0 || (is_nan(a) && is_nan(b)); }
template <typename T> std::uint64_t bits_of(T v) {
    std::uint64_t b = 0;
    std::memcpy(&b, &v, sizeof(T));
    return b;
}

// ---- views
struct Sl {
    int kind = 0;  // 0: SLICE_ALL, 1: SLICE(a, b) with a step, 2: an index (the axis is dropped)
    std::size_t a = 0, b = 0, step = 1;
};
struct ViewSpec {
    int slot = -1;
    bool transpose = false;
    std::vector<Sl> sl;  // empty: no subscript; else one per axis
    bool operator==(const ViewSpec &o) const {
        if (slot != o.slot || transpose != o.transpose || sl.size() != o.sl.size()) return false;
        for (std::size_t i = 0; i < sl.size(); ++i)
            if (sl[i].kind != o.sl[i].kind || sl[i].a != o.sl[i].a || sl[i].b != o.sl[i].b || sl[i].step != o.sl[i].step) return false;
        return true;
    }
};
struct View {
    int storage = -1;
    std::size_t offset = 0;
    Shape shape, strides;
    bool live() const { return storage >= 0; }
    std::size_t size() const { return prod(shape); }
    bool dense() const {
        std::size_t expect = 1;
        for (std::size_t i = shape.size(); i-- > 0;) {
            if (shape[i] != 1 && strides[i] != expect) return false;
            expect *= shape[i];
        }
        return true;
    }
    std::size_t last() const {  // the largest element offset it reaches, from `offset`
        std::size_t m = 0;
        for (std::size_t i = 0; i < shape.size(); ++i) m += (shape[i] - 1) * strides[i];
        return m;
    }
};
inline View apply_spec(const View &base, const ViewSpec &sp) {
    View v = base;
    if (sp.transpose) {
        v.shape.assign(base.shape.rbegin(), base.shape.rend());
        v.strides.assign(base.strides.rbegin(), base.strides.rend());
    }
    if (sp.sl.empty()) return v;
    View w;
    w.storage = v.storage, w.offset = v.offset;
    for (std::size_t d = 0; d < v.shape.size(); ++d) {
        const Sl s = d < sp.sl.size() ? sp.sl[d] : Sl{};
        if (s.kind == 0) {
            w.shape.push_back(v.shape[d]), w.strides.push_back(v.strides[d]);
        } else if (s.kind == 1) {
            w.offset += s.a * v.strides[d];
            w.shape.push_back((s.b - s.a + s.step - 1) / s.step), w.strides.push_back(v.strides[d] * s.step);
        } else {
            w.offset += s.a * v.strides[d];
        }
    }
    return w;
}
// f(linear, offset a, offset b) over `sh` in row-major order
template <typename F> void walk(const Shape &sh, const Shape &sa, const Shape &sb, F &&f) {
    const std::size_t n = prod(sh), nd = sh.size();
    std::vector<std::size_t> idx(nd, 0);
    std::size_t oa = 0, ob = 0;
    for (std::size_t lin = 0; lin < n; ++lin) {
        f(lin, oa, ob);
        for (std::size_t d = nd; d-- > 0;) {
            ++idx[d], oa += sa[d], ob += sb[d];
            if (idx[d] < sh[d]) break;
            oa -= sa[d] * sh[d], ob -= sb[d] * sh[d], idx[d] = 0;
        }
    }
}
// do the elements of b broadcast into shape a (aligned at the last axis)?
inline bool fits(const Shape &b, const Shape &a) {
    if (b.size() > a.size()) return false;
    const std::size_t pad = a.size() - b.size();
    for (std::size_t d = 0; d < b.size(); ++d)
        if (b[d] != a[pad + d] && b[d] != 1) return false;
    return true;
}
inline bool broadcast(const Shape &a, const Shape &b, Shape &out) {
    const std::size_t nd = a.size() > b.size() ? a.size() : b.size();
    out.assign(nd, 1);
    for (std::size_t d = 0; d < nd; ++d) {
        const std::size_t x = d + a.size() >= nd ? a[d + a.size() - nd] : 1, y = d + b.size() >= nd ? b[d + b.size() - nd] : 1;
        if (x != y && x != 1 && y != 1) return false;
        out[d] = x == 1 ? y : x;
    }
    return true;
}
inline Shape strides_over(const Shape &sh, const Shape &st, const Shape &over) {
    Shape r(over.size(), 0);
    const std::size_t pad = over.size() - sh.size();
    for (std::size_t d = 0; d < sh.size(); ++d) r[pad + d] = sh[d] == 1 ? 0 : st[d];
    return r;
}

template <typename T> struct Dense {
    Shape shape;
    std::vector<T> v;
};

// ---- expressions
enum NodeKind { N_LEAF, N_BIN, N_SCAL, N_LSCAL, N_NEG, N_ABS, N_SQRTABS, N_IPOW };
template <typename T> struct Node {
    int kind = N_LEAF, op = 0, a = -1, b = -1, k = 0;
    ViewSpec leaf;
    T scalar{};
};
template <typename T> struct Expr {
    std::vector<Node<T>> nodes;
    int root = -1, operators = 0;
};

// ---- statements
enum Kind {
    BIRTH_ONES, BIRTH_ZEROS, BIRTH_LIST, BIRTH_ADOPT, BIRTH_HOST_TINY, BIRTH_HOST_SMALL, VIEW_NEW,
    EXPR_NEW, ASSIGN, ASSIGN_TRANSPOSE, ASSIGN_SHIFTED, DISCARD, SUM_MEMBER, SUM_FREE,
    WRITE_DATA, WRITE_REF, WRITE_BULK, RESEED, READ_BURST, READ_CDATA, TO_STRING,
    ASSIGN_WHERE, PUT_ALONG_AXIS, FAMILY_MAX, FAMILY_ARGMAX, FAMILY_SORT, FAMILY_CUMMAX,
    DROP, DROP_RESULT, MOVE, CONTIGUOUS, REPEAT, REFUSED_EXPR, REFUSED_ROW, WRITE_MID, COMPARE, KIND_COUNT
};
inline const char *kind_name(int k) {
    static const char *names[] = {"birth ones * s", "birth zeros * s", "birth initializer list", "birth adopted new T[]", "birth host tiny <= 256 B",
                                  "birth host 257-1024 B", "view named", "auto r = E", "x<dst> = E", "x = x.transpose()", "x(0:k) = x(1:k+1) op E",
                                  "(void)(E)", "E.sum()", "sm::sum(E)", "x.data[i] = v", "x(i, j) = v", "bulk write through T*", "re-seed by host write",
                                  "as_const(x)(i, j) burst", "cdata()", "toString()", "assign_where", "put_along_axis + int64 index birth", "sm::max(E, axis)",
                                  "sm::argmax(E, axis)", "sm::sort(E, axis)", "sm::cummax(E, axis)", "drop", "drop a recorded result", "y = std::move(x)",
                                  "contiguous()", "repeat()", "refused: shape mismatch mid-expression", "refused: x(row) = wrong shape",
                                  "auto r = E op (write x, y): a write under a pending chain", "compare the pool"};
    return names[k];
}
enum DestForm { D_NONE, D_NEW, D_WHOLE, D_DENSE_BLOCK, D_STRIDED_BLOCK, D_ROW, D_VIEW_ENTRY, DEST_COUNT };
inline const char *dest_name(int d) {
    static const char *names[] = {"", "a new array", "a whole owner", "a dense block at an offset", "a strided block", "a single row (axis dropped)", "a named view"};
    return names[d];
}
enum Alias { A_NONE, A_IDENTICAL, A_OTHER_ORDER, A_SHIFTED, ALIAS_COUNT };
inline const char *alias_name(int a) {
    static const char *names[] = {"none", "identical block", "same storage in another order", "overlapping shifted"};
    return names[a];
}

template <typename T> struct Stmt {
    int kind = COMPARE;
    int slot = -1, slot2 = -1;      // the subject / destination entry; the entry that is born
    ViewSpec dst;                   // the subject seen through a subscript (slot == dst.slot)
    Expr<T> expr;
    bool fed_view = false;          // families: the operand is dst, not expr
    Shape shape;                    // births
    std::vector<T> values;          // births, host writes
    std::vector<std::size_t> at;    // host writes / reads: element positions (rank entries each for the (i, j) forms; storage-relative for data[i])
    std::vector<std::int64_t> index;  // put_along_axis: the index array, dense over index_shape
    Shape index_shape;
    T scalar{}, scalar2{};
    int axis = 0, op = 0, repeats = 1, variant = 0;
    // what the model says a run observes
    std::vector<T> expect;
    std::vector<std::int64_t> expect_index;
    Shape expect_shape;
    long double expect_sum = 0, sum_abs = 0;
    std::size_t sum_n = 0;
    // coverage
    int dest_form = D_NONE;
    bool alias[ALIAS_COUNT] = {};
    bool zero_ties_free = false;  // max / cummax: which zero a +-0 tie gives is not specified
};

struct Coverage {
    std::map<std::string, unsigned long long> rows;
    unsigned long long float_elements = 0, float_finite = 0, statements = 0, cases = 0;
    Coverage() {
        for (int k = 0; k < KIND_COUNT; ++k) rows[std::string("kind  ") + kind_name(k)] = 0;
        for (int d = 1; d < DEST_COUNT; ++d) rows[std::string("dest  ") + dest_name(d)] = 0;
        for (int a = 0; a < ALIAS_COUNT; ++a) rows[std::string("alias ") + alias_name(a)] = 0;
        for (int c = 0; c < 3; ++c) rows[std::string("class ") + class_name(c)] = 0;
        rows["expr  more than 8 leaves"] = 0;
        rows["expr  more than 4 array operands"] = 0;
        rows["expr  more than 8 operators"] = 0;
        rows["leaf  transposed"] = 0;
        rows["leaf  stepped"] = 0;
        rows["leaf  block at an offset"] = 0;
        rows["leaf  single row"] = 0;
        rows["leaf  broadcast"] = 0;
        rows["drop  an owner while a view lives"] = 0;
        rows["move  of a view"] = 0;
        rows["rank  1"] = rows["rank  2"] = rows["rank  3"] = rows["rank  4"] = 0;
    }
    void tick(const std::string &row) { ++rows[row]; }
    template <typename T> void count_compared(T v) {
        if constexpr (std::is_floating_point_v<T>) ++float_elements, float_finite += std::isfinite(v) ? 1 : 0;
        else (void)v;
    }
    void print(std::ostream &os) const {
        os << "coverage: " << cases << " cases, " << statements << " statements\n";
        for (const auto &r : rows) os << "  " << r.first << ": " << r.second << "\n";
        os << "finite: " << float_finite << " of " << float_elements << " compared float elements are finite in the model\n";
    }
};

// ---- the model
template <typename T> struct Model {
    static constexpr int kSlots = 12;
    std::vector<std::vector<T>> storages;
    View pool[kSlots];

    int live_count() const {
        int n = 0;
        for (const View &v : pool) n += v.live();
        return n;
    }
    int free_slot() const {
        for (int i = 0; i < kSlots; ++i)
            if (!pool[i].live()) return i;
        return -1;
    }
    int users(int storage) const {
        int n = 0;
        for (const View &v : pool) n += v.storage == storage;
        return n;
    }
    void release(int slot) {
        const int st = pool[slot].storage;
        pool[slot] = View{};
        if (st >= 0 && users(st) == 0) std::vector<T>().swap(storages[st]);
    }
    int birth(int slot, const Shape &shape, std::vector<T> &&values) {
        storages.push_back(std::move(values));
        pool[slot] = View{static_cast<int>(storages.size()) - 1, 0, shape, dense_strides(shape)};
        return slot;
    }
    View view(const ViewSpec &sp) const { return apply_spec(pool[sp.slot], sp); }
    Dense<T> read(const View &w) const {
        Dense<T> d{w.shape, std::vector<T>(w.size())};
        const T *base = storages[w.storage].data() + w.offset;
        walk(w.shape, w.strides, w.strides, [&](std::size_t lin, std::size_t o, std::size_t) { d.v[lin] = base[o]; });
        return d;
    }
    void store(const View &w, const Dense<T> &d) {  // d broadcasts into w
        T *base = storages[w.storage].data() + w.offset;
        const Shape sd = strides_over(d.shape, dense_strides(d.shape), w.shape);
        walk(w.shape, w.strides, sd, [&](std::size_t, std::size_t o, std::size_t od) { base[o] = d.v[od]; });
    }
    Dense<T> binary(int op, const Dense<T> &a, const Dense<T> &b) const {
        Dense<T> r;
        broadcast(a.shape, b.shape, r.shape);
        r.v.resize(prod(r.shape));
        const Shape sa = strides_over(a.shape, dense_strides(a.shape), r.shape), sb = strides_over(b.shape, dense_strides(b.shape), r.shape);
        walk(r.shape, sa, sb, [&](std::size_t lin, std::size_t oa, std::size_t ob) { r.v[lin] = arith<T>(op, a.v[oa], b.v[ob]); });
        return r;
    }
    Dense<T> eval(const Expr<T> &e, int at) const {
        const Node<T> &n = e.nodes[at];
        switch (n.kind) {
            case N_LEAF: return read(view(n.leaf));
            case N_BIN: {
                const Dense<T> a = eval(e, n.a), b = eval(e, n.b);
                return binary(n.op, a, b);
            }
            case N_SCAL: {
                Dense<T> a = eval(e, n.a);
                for (T &x : a.v) x = arith<T>(n.op, x, n.scalar);
                return a;
            }
            case N_LSCAL: {  // SMArray<T>{s} op a: a one-element array on the left
                Dense<T> a = eval(e, n.a);
                for (T &x : a.v) x = arith<T>(n.op, n.scalar, x);
                return a;
            }
            default: {
                Dense<T> a = eval(e, n.a);
                for (T &x : a.v)
                    x = n.kind == N_NEG ? Ar<T>::neg(x) : n.kind == N_ABS ? Ar<T>::abs(x) : n.kind == N_SQRTABS ? Ar<T>::sqrtabs(x) : Ar<T>::ipow(x, n.k);
                return a;
            }
        }
    }
    Dense<T> eval(const Expr<T> &e) const { return eval(e, e.root); }
};

// how `leaf` lies against `dst` in the same storage
inline int alias_of(const View &dst, const View &leaf, std::size_t storage_size) {
    if (dst.storage != leaf.storage) return A_NONE;
    if (dst.offset == leaf.offset && dst.shape == leaf.shape && dst.strides == leaf.strides) return A_IDENTICAL;
    std::vector<unsigned char> mark(storage_size, 0);
    walk(dst.shape, dst.strides, dst.strides, [&](std::size_t, std::size_t o, std::size_t) { mark[dst.offset + o] = 1; });
    bool overlap = false;
    walk(leaf.shape, leaf.strides, leaf.strides, [&](std::size_t, std::size_t o, std::size_t) { overlap |= mark[leaf.offset + o] != 0; });
    if (!overlap) return A_NONE;
    return dst.shape == leaf.shape && dst.strides == leaf.strides ? A_SHIFTED : A_OTHER_ORDER;
}

// ---- text
inline std::string text_of(const ViewSpec &sp) {
    std::ostringstream os;
    os << "v" << sp.slot;
    if (sp.transpose) os << ".transpose()";
    if (!sp.sl.empty()) {
        os << "(";
        for (std::size_t i = 0; i < sp.sl.size(); ++i) {
            const Sl &s = sp.sl[i];
            if (i) os << ", ";
            if (s.kind == 0) os << "SLICE_ALL";
            else if (s.kind == 2) os << s.a;
            else if (s.step == 1) os << "SLICE(" << s.a << ", " << s.b << ")";
            else os << "SLICE(" << s.a << ", " << s.b << ", step " << s.step << ")";
        }
        os << ")";
    }
    return os.str();
}
template <typename T> std::string num_text(T v) {
    std::ostringstream os;
    os.precision(std::numeric_limits<T>::max_digits10);
    os << v;
    return os.str();
}
inline std::string text_of(const Shape &s) {
    std::ostringstream os;
    os << "{";
    for (std::size_t i = 0; i < s.size(); ++i) os << (i ? ", " : "") << s[i];
    os << "}";
    return os.str();
}
template <typename T> std::string text_of(const Expr<T> &e, int at) {
    static const char *ops[] = {" + ", " - ", " * ", " / "};
    const Node<T> &n = e.nodes[at];
    switch (n.kind) {
        case N_LEAF: return text_of(n.leaf);
        case N_BIN: return "(" + text_of(e, n.a) + ops[n.op] + text_of(e, n.b) + ")";
        case N_SCAL: return "(" + text_of(e, n.a) + ops[n.op] + num_text(n.scalar) + ")";
        case N_LSCAL: return "(SMArray<T>{" + num_text(n.scalar) + "}" + ops[n.op] + text_of(e, n.a) + ")";
        case N_NEG: return "-" + text_of(e, n.a);
        case N_ABS: return "sm::abs(" + text_of(e, n.a) + ")";
        case N_SQRTABS: return "sm::sqrt(sm::abs(" + text_of(e, n.a) + "))";
        default: return "sm::pow(" + text_of(e, n.a) + ", " + std::to_string(n.k) + ")";
    }
}
template <typename T> std::string text_of(const Stmt<T> &s) {
    std::ostringstream os;
    const std::string E = s.expr.root >= 0 ? text_of(s.expr, s.expr.root) : std::string();
    const std::string operand = s.fed_view ? text_of(s.dst) : E;
    switch (s.kind) {
        case BIRTH_ONES: os << "auto v" << s.slot2 << " = sm::ones<T>" << text_of(s.shape) << " * " << num_text(s.scalar) << ";"; break;
        case BIRTH_ZEROS: os << "auto v" << s.slot2 << " = sm::zeros<T>" << text_of(s.shape) << " * " << num_text(s.scalar) << ";"; break;
        case BIRTH_LIST: os << "SMArray<T> v" << s.slot2 << "{" << s.values.size() << " values from " << num_text(s.values[0]) << "};  // shape " << text_of(s.shape); break;
        case BIRTH_ADOPT: case BIRTH_HOST_TINY: case BIRTH_HOST_SMALL:
            os << "SMArray<T> v" << s.slot2 << "(new T[" << s.values.size() << "]{" << num_text(s.values[0]) << ", ...}, " << text_of(s.shape) << ");"; break;
        case VIEW_NEW: os << "auto v" << s.slot2 << " = " << text_of(s.dst) << ";"; break;
        case EXPR_NEW: os << "auto v" << s.slot2 << " = " << E << ";"; break;
        case ASSIGN: case ASSIGN_SHIFTED: case REFUSED_ROW: os << text_of(s.dst) << " = " << E << ";" << (s.kind == REFUSED_ROW ? "  // throws" : ""); break;
        case ASSIGN_TRANSPOSE: os << "v" << s.slot << " = v" << s.slot << ".transpose();"; break;
        case DISCARD: os << "(void)(" << E << ");"; break;
        case REFUSED_EXPR: os << "(void)(" << E << ");  // throws"; break;
        case SUM_MEMBER: os << "(" << E << ").sum();"; break;
        case SUM_FREE: os << "sm::sum(" << E << ");"; break;
        case WRITE_DATA: os << "v" << s.slot << ".data[" << s.at[0] << "] = " << num_text(s.values[0]) << ";  // " << s.values.size() << " such"; break;
        case WRITE_REF: os << "v" << s.slot << "(" << s.at[0] << ", ...) = " << num_text(s.values[0]) << ";  // " << s.values.size() << " such"; break;
        case WRITE_BULK: case RESEED:
            os << "T *p = static_cast<T *>(v" << s.slot << ".data) - " << s.at[0] << "; for (i < " << s.values.size() << ") p[" << s.at[1] << " + i] = ...;"; break;
        case READ_BURST: os << "std::as_const(v" << s.slot << ")(" << s.at[0] << ", ...);  // " << s.expect.size() << " reads"; break;
        case READ_CDATA: os << "v" << s.slot << ".cdata();"; break;
        case TO_STRING: os << text_of(s.dst) << ".toString();"; break;
        case ASSIGN_WHERE: os << text_of(s.dst) << ".assign_where(" << text_of(s.dst) << " > " << num_text(s.scalar) << ", " << num_text(s.scalar2) << ");"; break;
        case PUT_ALONG_AXIS: os << text_of(s.dst) << ".put_along_axis(SMArray<int64_t>(host, " << text_of(s.index_shape) << "), " << num_text(s.scalar) << ", " << s.axis << ");"; break;
        case FAMILY_MAX: os << "sm::max(" << operand << ", " << s.axis << ");"; break;
        case FAMILY_ARGMAX: os << "sm::argmax(" << operand << ", " << s.axis << ");"; break;
        case FAMILY_SORT: os << "sm::sort(" << operand << ", " << s.axis << ");"; break;
        case FAMILY_CUMMAX: os << "sm::cummax(" << operand << ", " << s.axis << ");"; break;
        case DROP: os << "drop v" << s.slot << ";"; break;
        case DROP_RESULT: os << "{ auto r = " << E << "; }"; break;
        case MOVE: os << "SMArray<T> v" << s.slot2 << " = std::move(v" << s.slot << ");"; break;
        case CONTIGUOUS: os << "auto v" << s.slot2 << " = " << text_of(s.dst) << ".contiguous();"; break;
        case REPEAT: os << text_of(s.dst) << ".repeat(" << s.repeats << ");"; break;
        case WRITE_MID:
            os << "auto v" << s.slot2 << " = " << E << " op" << s.op << " (";
            if (s.variant == 0) os << "v" << s.slot << ".data[" << s.at[0] << "] = " << num_text(s.values[0]);
            else os << "v" << s.slot << ".assign_where(v" << s.slot << " > " << num_text(s.scalar) << ", " << num_text(s.scalar2) << ")";
            os << ", " << text_of(s.dst) << ");";
            break;
        default: os << "compare the pool;"; break;
    }
    return os.str();
}

// ---- JSON (values as bit patterns, so that a replay elsewhere starts from the same bits)
inline void json_of(std::ostream &os, const Shape &s) {
    os << "[";
    for (std::size_t i = 0; i < s.size(); ++i) os << (i ? "," : "") << s[i];
    os << "]";
}
template <typename T> void json_bits(std::ostream &os, const std::vector<T> &v) {
    os << "[";
    for (std::size_t i = 0; i < v.size(); ++i) os << (i ? "," : "") << bits_of(v[i]);
    os << "]";
}
inline void json_of(std::ostream &os, const ViewSpec &sp) {
    os << "{\"slot\":" << sp.slot << ",\"t\":" << (sp.transpose ? 1 : 0) << ",\"sl\":[";
    for (std::size_t i = 0; i < sp.sl.size(); ++i) os << (i ? "," : "") << "[" << sp.sl[i].kind << "," << sp.sl[i].a << "," << sp.sl[i].b << "," << sp.sl[i].step << "]";
    os << "]}";
}
template <typename T> void json_of(std::ostream &os, const Expr<T> &e) {
    os << "{\"root\":" << e.root << ",\"nodes\":[";
    for (std::size_t i = 0; i < e.nodes.size(); ++i) {
        const Node<T> &n = e.nodes[i];
        os << (i ? "," : "") << "{\"kind\":" << n.kind << ",\"op\":" << n.op << ",\"a\":" << n.a << ",\"b\":" << n.b << ",\"k\":" << n.k << ",\"scalar\":" << bits_of(n.scalar) << ",\"leaf\":";
        json_of(os, n.leaf);
        os << "}";
    }
    os << "]}";
}
template <typename T> void json_of(std::ostream &os, const Stmt<T> &s) {
    os << "{\"kind\":" << s.kind << ",\"slot\":" << s.slot << ",\"slot2\":" << s.slot2 << ",\"dst\":";
    json_of(os, s.dst);
    os << ",\"expr\":";
    json_of(os, s.expr);
    os << ",\"shape\":";
    json_of(os, s.shape);
    os << ",\"values\":";
    json_bits(os, s.values);
    os << ",\"at\":";
    json_of(os, s.at);
    os << ",\"index\":[";
    for (std::size_t i = 0; i < s.index.size(); ++i) os << (i ? "," : "") << s.index[i];
    os << "],\"index_shape\":";
    json_of(os, s.index_shape);
    os << ",\"scalar\":" << bits_of(s.scalar) << ",\"scalar2\":" << bits_of(s.scalar2) << ",\"axis\":" << s.axis << ",\"op\":" << s.op << ",\"variant\":" << s.variant << ",\"text\":\"" << text_of(s) << "\"}";
}
template <typename T> void json_pool(std::ostream &os, const Model<T> &m) {
    os << "[";
    bool first = true;
    for (int i = 0; i < Model<T>::kSlots; ++i) {
        if (!m.pool[i].live()) continue;
        os << (first ? "" : ",") << "{\"slot\":" << i << ",\"shape\":";
        json_of(os, m.pool[i].shape);
        os << ",\"bits\":";
        json_bits(os, m.read(m.pool[i]).v);
        os << "}";
        first = false;
    }
    os << "]";
}

// ---- the generator
template <typename T> class Case {
public:
    static constexpr bool kFloat = std::is_floating_point_v<T>;
    Model<T> model;
    int size_class;

    Case(std::uint64_t seed, std::uint64_t k, Coverage &cov) : size_class(class_of_case(k)), rng{case_seed(seed, k)}, cov_(cov) {
        draw_shapes();
        budget_ = size_class == TINY ? 44 : size_class == SMALL ? 32 : 14;
        ++cov_.cases;
        cov_.tick(std::string("class ") + class_name(size_class));
        cov_.tick("rank  " + std::to_string(base_.size()));
    }

    // The next statement, already applied to the model; false when the case is over (its last statement is a COMPARE).
    bool next(Stmt<T> &out) {
        if (done_) return false;
        out = Stmt<T>{};
        if (reseed(out)) {
        } else if (emitted_ >= budget_) {
            done_ = true;  // the whole pool is compared at the end of every case
        } else if (compare_due_) {
            compare_due_ = false;
        } else {
            draw(out);
            ++emitted_;
            compare_due_ = rng.chance(1, 8);
        }
        ++cov_.statements;
        cov_.tick(std::string("kind  ") + kind_name(out.kind));
        if (out.dest_form != D_NONE) cov_.tick(std::string("dest  ") + dest_name(out.dest_form));
        if (out.kind == ASSIGN || out.kind == ASSIGN_SHIFTED || out.kind == ASSIGN_TRANSPOSE)
            for (int a = 0; a < ALIAS_COUNT; ++a)
                if (out.alias[a]) cov_.tick(std::string("alias ") + alias_name(a));
        if (out.kind == COMPARE)
            for (const View &v : model.pool)
                if (v.live())
                    for (T x : model.read(v).v) cov_.count_compared(x);
        for (T x : out.expect) cov_.count_compared(x);
        return true;
    }

private:
    Rng rng;
    Coverage &cov_;
    Shape base_, row_, col_, one_, trans_, parent_;
    int budget_ = 0, emitted_ = 0;
    bool done_ = false, compare_due_ = false;

    // ---- shapes: a base (.., R, C) with its row, column, (1, 1), transposed and taller companions
    void draw_shapes() {
        std::size_t R, C;
        if (size_class == TINY) {
            C = rng.chance(1, 4) ? rng.range(1, 6) : rng.range(7, 130);
            R = rng.range(1, 4096 / C > 40 ? 40 : 4096 / C);
            if (rng.chance(1, 3)) R = C = rng.range(2, 48);  // square: x = x.transpose()
        } else if (size_class == SMALL) {
            C = rng.range(65, 300);
            R = rng.range(4097 / C + 1, 65536 / C > 200 ? 200 : 65536 / C);
            if (rng.chance(1, 3)) R = C = rng.range(65, 255);
        } else {
            const std::size_t elements = (std::size_t{1} << 20) / sizeof(T);  // 1 MiB of results and a little more
            C = rng.range(257, 600) | 1;
            R = elements / C + 2;
        }
        base_ = {R, C};
        const std::size_t rank = size_class == MID ? 2 : rng.chance(2, 5) ? 2 : rng.chance(1, 3) ? 1 : rng.range(3, 4);
        if (rank == 1) base_ = {size_class == TINY ? rng.range(1, 4096) : R * C};
        else if (rank == 3) base_ = rng.chance(1, 2) ? Shape{R, 1, C} : Shape{rng.chance(1, 2) ? std::size_t{1} : R / 2 + 1, 2, C > 2 ? C / 2 : 1};
        else if (rank == 4) base_ = Shape{rng.range(1, 2), R > 4 ? R / 4 : 1, rng.range(1, 2), C > 2 ? C / 2 : 1};
        if (size_class == SMALL && prod(base_) <= 4096) base_[0] = 4097 / (prod(base_) / base_[0]) + 1;
        const std::size_t nd = base_.size();
        row_ = rng.chance(1, 2) ? Shape{base_[nd - 1]} : Shape(nd, 1);
        row_.back() = base_[nd - 1];
        col_ = base_;
        col_.back() = 1;
        one_ = rng.chance(1, 2) ? Shape{1} : Shape(nd, 1);
        trans_.assign(base_.rbegin(), base_.rend());
        parent_ = base_;
        parent_[0] = 2 * base_[0] + 1;
    }

    T draw_value() {
        const std::size_t r = rng.below(100);
        if constexpr (kFloat) {
            if (r < 1) return T(0);
            if (r < 2) return -T(0);
            if (r < 10) return static_cast<T>(static_cast<int>(rng.below(17)) - 8);
            const T m = static_cast<T>(static_cast<double>(rng.next() >> 11) * (1.0 / 9007199254740992.0) * 4.0 - 2.0);
            if (r < 16) return m * static_cast<T>(r < 13 ? 1048576.0 : 1.0 / 1048576.0);
            return m;
        } else {
            if (r < 4) return 0;
            if (r < 8) return r < 6 ? T(1) : T(-1);
            if (r < 10) return r < 9 ? std::numeric_limits<T>::min() : std::numeric_limits<T>::max();
            if (r < 14) return static_cast<T>(static_cast<std::int32_t>(rng.next()));
            return static_cast<T>(static_cast<int>(rng.below(19)) - 9);
        }
    }
    T draw_scalar() {
        if constexpr (kFloat) return static_cast<T>((static_cast<int>(rng.below(31)) - 15) * 0.25 + (rng.chance(1, 2) ? 0.125 : 0.3));
        else return static_cast<T>(static_cast<int>(rng.below(9)) - 4);
    }
    std::vector<T> draw_values(std::size_t n) {
        std::vector<T> v(n);
        for (T &x : v) x = draw_value();
        return v;
    }
    int random_live() {
        int live[Model<T>::kSlots], n = 0;
        for (int i = 0; i < Model<T>::kSlots; ++i)
            if (model.pool[i].live()) live[n++] = i;
        return n ? live[rng.below(n)] : -1;
    }
    bool is_owner(int slot) const {
        const View &e = model.pool[slot];
        return e.offset == 0 && e.dense() && e.size() == model.storages[e.storage].size();
    }
    int random_live_preferring_views() {  // one time in three a named view, if one is found
        int slot = random_live();
        if (rng.chance(1, 3))
            for (int attempt = 0; attempt < 4 && slot >= 0 && is_owner(slot); ++attempt) slot = random_live();
        return slot;
    }
    const Shape &companion(std::size_t i) const { return i == 0 ? base_ : i == 1 ? row_ : i == 2 ? col_ : i == 3 ? one_ : i == 4 ? trans_ : parent_; }

    // ---- re-seeding: a stored array with an element that is not finite, or outside 2^+-60, is written anew by the next statement
    bool reseed(Stmt<T> &s) {
        if constexpr (kFloat) {
            for (int i = 0; i < Model<T>::kSlots; ++i) {
                const View &v = model.pool[i];
                if (!v.live()) continue;
                std::vector<T> &st = model.storages[v.storage];
                bool bad = false;
                for (T x : st) bad |= !std::isfinite(x) || (x != 0 && (std::fabs(x) > T(1.15e18) || std::fabs(x) < T(8.7e-19)));
                if (!bad) continue;
                s.kind = RESEED, s.slot = i, s.at = {v.offset, 0}, s.values = draw_values(st.size());
                st = s.values;
                return true;
            }
        }
        (void)s;
        return false;
    }

    // ---- views of an entry that fit a target shape
    // form 0 whole, 1 transposed, 2 block of the first axis at an offset, 3 stepped, 4 one index of the first axis (axis dropped),
    // 5 one row kept as an extent of 1, 6 one column
    bool make_spec(int slot, int form, const Shape &target, bool exact, ViewSpec &sp) {
        const View &e = model.pool[slot];
        const std::size_t r = e.shape.size();
        sp = ViewSpec{};
        sp.slot = slot;
        if (form == 1) {
            if (r < 2) return false;
            sp.transpose = true;
        } else if (form >= 2) {
            sp.sl.assign(r, Sl{});
            if (form == 6) {
                sp.sl[r - 1] = Sl{1, rng.below(e.shape[r - 1]), 0, 1};
                sp.sl[r - 1].b = sp.sl[r - 1].a + 1;
            } else if (form == 4) {
                if (r < 2) return false;
                sp.sl[0] = Sl{2, rng.below(e.shape[0]), 0, 1};
            } else if (form == 5) {
                sp.sl[0] = Sl{1, rng.below(e.shape[0]), 0, 1};
                sp.sl[0].b = sp.sl[0].a + 1;
            } else {
                if (r > target.size()) return false;
                const std::size_t n = target[target.size() - r], have = e.shape[0];
                if (form == 2) {
                    if (have <= n || n == 0) return false;
                    const std::size_t a = rng.range(1, have - n);
                    sp.sl[0] = Sl{1, a, a + n, 1};
                } else {
                    if (have < 2 * n || n == 0) return false;
                    const std::size_t a = rng.range(0, have - (2 * n - 1));
                    sp.sl[0] = Sl{1, a, a + 2 * n - 1, 2};
                }
            }
        }
        const View v = model.view(sp);
        if (v.shape.empty()) return false;
        return exact ? v.shape == target : fits(v.shape, target);
    }
    bool draw_leaf(const Shape &target, bool exact, int prefer_storage, ViewSpec &sp) {
        for (int attempt = 0; attempt < 40; ++attempt) {
            const int slot = random_live();
            if (slot < 0) return false;
            if (prefer_storage >= 0 && attempt < 20 && model.pool[slot].storage != prefer_storage) continue;
            const int form = rng.chance(2, 5) ? 0 : static_cast<int>(rng.below(7));
            if (make_spec(slot, form, target, exact, sp)) return true;
        }
        return false;
    }

    // ---- expressions: a random tree of `operators` operators whose value has exactly the shape `target`
    int grow(Expr<T> &e, int operators, const Shape &target, bool exact, int prefer_storage, const ViewSpec *same) {
        Node<T> n;
        if (operators <= 0) {
            if (same && exact && rng.chance(1, 3)) n.leaf = *same;
            else if (!draw_leaf(target, exact, rng.chance(1, 3) ? prefer_storage : -1, n.leaf)) return -1;
            e.nodes.push_back(n);
            return static_cast<int>(e.nodes.size()) - 1;
        }
        const std::size_t pick = rng.below(10);
        if (pick < 5 && operators >= 1) {  // array op array
            n.kind = N_BIN, n.op = static_cast<int>(rng.below(4));
            const int left = static_cast<int>(rng.below(operators));  // operators - 1 to share
            const bool full_left = rng.chance(3, 4);
            n.a = grow(e, left, target, exact && full_left, prefer_storage, same);
            n.b = grow(e, operators - 1 - left, target, exact && !full_left, prefer_storage, same);
            if (n.a < 0 || n.b < 0) return -1;
        } else if (pick < 7) {
            n.kind = rng.chance(1, 3) ? N_LSCAL : N_SCAL, n.op = static_cast<int>(rng.below(4)), n.scalar = draw_scalar();
            if (n.kind == N_SCAL && n.op == 3 && n.scalar == T(0)) n.scalar = T(2);
            n.a = grow(e, operators - 1, target, exact, prefer_storage, same);
        } else {
            if constexpr (kFloat) {
                n.kind = pick == 7 ? N_NEG : pick == 8 ? N_ABS : N_SQRTABS;
                if (n.kind == N_SQRTABS && operators < 2) n.kind = N_ABS;
            } else {
                n.kind = pick == 7 ? N_NEG : pick == 8 ? N_ABS : N_IPOW, n.k = static_cast<int>(rng.below(4));
            }
            n.a = grow(e, operators - (n.kind == N_SQRTABS ? 2 : 1), target, exact, prefer_storage, same);
        }
        if (n.a < 0) return -1;
        e.nodes.push_back(n);
        return static_cast<int>(e.nodes.size()) - 1;
    }
    // ... mostly finite in the model; the leaves are counted for the coverage table
    bool draw_expr(Expr<T> &e, const Shape &target, int prefer_storage, const ViewSpec *same, int min_ops = 1) {
        for (int attempt = 0; attempt < 6; ++attempt) {
            e = Expr<T>{};
            const std::size_t r = rng.below(10);
            e.operators = static_cast<int>(r < 4 ? rng.range(1, 3) : r < 8 ? rng.range(3, 8) : rng.range(9, 12));
            if (e.operators < min_ops) e.operators = min_ops;
            e.root = grow(e, e.operators, target, true, prefer_storage, same);
            if (e.root < 0) continue;
            if (model.eval(e).shape != target) continue;
            if (!mostly_finite(model.eval(e).v)) continue;
            return true;
        }
        return false;
    }
    static bool mostly_finite(const std::vector<T> &v) {
        std::size_t bad = 0;
        for (T x : v) bad += !is_finite(x);
        return bad * 50 <= v.size();
    }
    void count_leaves(const Expr<T> &e) {
        int leaves = 0, arrays = 0;
        const std::size_t results = prod(model.eval(e).shape);
        for (const Node<T> &n : e.nodes) {
            leaves += n.kind == N_LEAF || n.kind == N_SCAL || n.kind == N_LSCAL;
            if (n.kind != N_LEAF) continue;
            ++arrays;
            const View v = model.view(n.leaf);
            if (n.leaf.transpose) cov_.tick("leaf  transposed");
            for (const Sl &s : n.leaf.sl) {
                if (s.kind == 1 && s.step > 1) cov_.tick("leaf  stepped");
                else if (s.kind == 1 && s.a > 0 && s.b - s.a > 1) cov_.tick("leaf  block at an offset");
                else if (s.kind == 2) cov_.tick("leaf  single row");
            }
            if (v.size() < results) cov_.tick("leaf  broadcast");
        }
        if (leaves > 8) cov_.tick("expr  more than 8 leaves");
        if (arrays > 4) cov_.tick("expr  more than 4 array operands");
        if (e.operators > 8) cov_.tick("expr  more than 8 operators");
    }
    void classify(Stmt<T> &s, const View &dst) {
        for (const Node<T> &n : s.expr.nodes)
            if (n.kind == N_LEAF) s.alias[alias_of(dst, model.view(n.leaf), model.storages[dst.storage].size())] = true;
        bool any = false;
        for (int a = 1; a < ALIAS_COUNT; ++a) any |= s.alias[a];
        s.alias[A_NONE] = !any;
    }

    // ---- one statement
    void draw(Stmt<T> &s) {
        if (emitted_ < 7) {  // the case opens with one array of every companion shape, two of the base
            birth(s, emitted_ < 2 ? 0 : emitted_ - 1, true);
            return;
        }
        for (int attempt = 0; attempt < 30; ++attempt) {
            s = Stmt<T>{};
            if (try_draw(s)) return;
        }
        s = Stmt<T>{};
        if (model.free_slot() < 0) drop(s);
        else birth(s, 0);
    }
    bool try_draw(Stmt<T> &s) {
        const int live = model.live_count();
        if (live >= Model<T>::kSlots - 1) return drop(s);
        const std::size_t r = rng.below(100);
        if (r < 8) return birth(s, rng.below(6));
        if (r < 12) return view_new(s);
        if (r < 20) return expr_new(s);
        if (r < 38) return assign(s);
        if (r < 43) return assign_transpose(s);
        if (r < 47) return assign_shifted(s);
        if (r < 49) return with_expr(s, DISCARD);
        if (r < 53) return sum(s);
        if (r < 62) return host_write(s);
        if (r < 69) return host_read(s);
        if (r < 73) return assign_where(s);
        if (r < 76) return put_along_axis(s);
        if (r < 84) return family(s);
        if (r < 86) return drop(s);
        if (r < 88) return with_expr(s, DROP_RESULT);
        if (r < 92) return move(s);
        if (r < 94) return contiguous(s);
        if (r < 96) return repeat(s);
        if (r < 98) return write_mid(s);
        return refused(s);
    }

    bool birth(Stmt<T> &s, std::size_t which, bool opening = false) {
        const int slot = model.free_slot();
        if (slot < 0) return false;
        s.slot2 = slot, s.dest_form = D_NEW;
        const std::size_t r = opening ? rng.below(3) + 7 * rng.below(2) : rng.below(10);
        const std::size_t bytes_tiny = 256 / sizeof(T), bytes_small = 1024 / sizeof(T);
        s.shape = companion(which);
        if (r < 2) {
            s.kind = BIRTH_ONES, s.scalar = draw_scalar();
            s.values.assign(prod(s.shape), Ar<T>::mul(T(1), s.scalar));
        } else if (r < 3) {
            s.kind = BIRTH_ZEROS, s.scalar = draw_scalar();
            s.values.assign(prod(s.shape), Ar<T>::mul(T(0), s.scalar));
        } else if (r < 5) {  // an initializer list: the row when it has at most 6 elements, {2, 3} of them, or one element
            s.kind = BIRTH_LIST;
            s.shape = row_.back() <= 6 ? Shape{row_.back()} : base_ == Shape{2, 3} ? base_ : Shape{1};
            s.values = draw_values(prod(s.shape));
        } else if (r < 7) {  // host-built, small enough to ride in a launch packet: whichever companion has the size
            s.kind = r < 6 ? BIRTH_HOST_TINY : BIRTH_HOST_SMALL;
            bool found = false;
            for (std::size_t i = 0; i < 6 && !found; ++i) {
                const Shape &c = companion((which + i) % 6);
                const std::size_t n = prod(c);
                if (s.kind == BIRTH_HOST_TINY ? n <= bytes_tiny : (n > bytes_tiny && n <= bytes_small)) s.shape = c, found = true;
            }
            if (!found) s.kind = BIRTH_ADOPT;
            s.values = draw_values(prod(s.shape));
        } else {
            s.kind = BIRTH_ADOPT;
            s.values = draw_values(prod(s.shape));
        }
        model.birth(slot, s.shape, std::vector<T>(s.values));
        return true;
    }
    bool view_new(Stmt<T> &s) {
        const int slot = model.free_slot(), from = random_live();
        if (slot < 0 || from < 0) return false;
        const View &e = model.pool[from];
        const int form = static_cast<int>(rng.range(1, 6));
        Shape target = e.shape;  // forms 2 and 3 take half of the first axis
        target[0] = e.shape[0] / 2;
        if (!make_spec(from, form, target, false, s.dst) && !make_spec(from, 5, e.shape, false, s.dst)) return false;
        s.kind = VIEW_NEW, s.slot = from, s.slot2 = slot, s.dest_form = D_NEW;
        model.pool[slot] = model.view(s.dst);
        return true;
    }
    bool expr_new(Stmt<T> &s) {
        const int slot = model.free_slot();
        if (slot < 0) return false;
        const Shape target = rng.chance(3, 4) ? base_ : model.pool[random_live()].shape;
        if (!draw_expr(s.expr, target, -1, nullptr)) return false;
        count_leaves(s.expr);
        s.kind = EXPR_NEW, s.slot2 = slot, s.dest_form = D_NEW;
        Dense<T> d = model.eval(s.expr);
        model.birth(slot, d.shape, std::move(d.v));
        return true;
    }
    // a destination: an entry as it is, a dense block of it at an offset, a strided block, one row
    bool draw_destination(Stmt<T> &s) {
        const int slot = random_live_preferring_views();
        if (slot < 0) return false;
        const View &e = model.pool[slot];
        s.slot = slot, s.dst = ViewSpec{};
        s.dst.slot = slot;
        const std::size_t r = rng.below(10), nd = e.shape.size();
        if (r < 4) {
            s.dest_form = e.offset == 0 && e.dense() && e.size() == model.storages[e.storage].size() ? D_WHOLE : D_VIEW_ENTRY;
        } else if (r < 6) {  // rows a .. b of the first axis: dense when the entry is
            if (e.shape[0] < 3) return false;
            const std::size_t a = rng.range(1, e.shape[0] - 2), b = rng.range(a + 1, e.shape[0] - 1);
            s.dst.sl.assign(nd, Sl{});
            s.dst.sl[0] = Sl{1, a, b, 1};
            s.dest_form = e.dense() ? D_DENSE_BLOCK : D_STRIDED_BLOCK;
        } else if (r < 8) {  // columns a .. b, or every second row
            s.dst.sl.assign(nd, Sl{});
            if (rng.chance(1, 2) && e.shape[nd - 1] >= 3) {
                const std::size_t a = rng.range(0, e.shape[nd - 1] - 2);
                s.dst.sl[nd - 1] = Sl{1, a, rng.range(a + 1, e.shape[nd - 1] - 1), 1};
            } else {
                if (e.shape[0] < 3) return false;
                s.dst.sl[0] = Sl{1, rng.below(2), e.shape[0], 2};
            }
            s.dest_form = D_STRIDED_BLOCK;
        } else {
            if (nd < 2) return false;
            s.dst.sl.assign(nd, Sl{});
            s.dst.sl[0] = Sl{2, rng.below(e.shape[0]), 0, 1};
            s.dest_form = D_ROW;
        }
        const View v = model.view(s.dst);
        return !v.shape.empty() && v.size() != 0;
    }
    bool assign(Stmt<T> &s) {
        if (!draw_destination(s)) return false;
        const View dst = model.view(s.dst);
        if (!draw_expr(s.expr, dst.shape, dst.storage, &s.dst)) return false;
        count_leaves(s.expr);
        s.kind = ASSIGN;
        classify(s, dst);
        model.store(dst, model.eval(s.expr));
        return true;
    }
    bool assign_transpose(Stmt<T> &s) {
        for (int attempt = 0; attempt < 8; ++attempt) {
            const int slot = random_live();
            const View &e = model.pool[slot];
            if (e.shape.size() != 2 || e.shape[0] != e.shape[1] || e.shape[0] < 2) continue;
            s.kind = ASSIGN_TRANSPOSE, s.slot = slot, s.dest_form = D_WHOLE, s.alias[A_OTHER_ORDER] = true;
            ViewSpec t;
            t.slot = slot, t.transpose = true;
            model.store(e, model.read(model.view(t)));
            return true;
        }
        return false;
    }
    bool assign_shifted(Stmt<T> &s) {
        const int slot = random_live();
        const View &e = model.pool[slot];
        if (e.shape[0] < 3) return false;
        const std::size_t nd = e.shape.size(), k = rng.range(2, e.shape[0] - 1);
        const bool up = rng.chance(1, 2);
        s.slot = slot, s.dst.slot = slot;
        s.dst.sl.assign(nd, Sl{});
        s.dst.sl[0] = up ? Sl{1, 1, k + 1, 1} : Sl{1, 0, k, 1};
        ViewSpec from = s.dst;
        from.sl[0] = up ? Sl{1, 0, k, 1} : Sl{1, 1, k + 1, 1};
        const View dst = model.view(s.dst);
        Expr<T> rest;
        const bool with_rest = rng.chance(2, 3) && draw_expr(rest, dst.shape, dst.storage, nullptr);
        Node<T> leaf;
        leaf.leaf = from;
        s.expr = with_rest ? rest : Expr<T>{};
        s.expr.nodes.push_back(leaf);
        Node<T> top;
        top.op = static_cast<int>(rng.below(3)), top.a = static_cast<int>(s.expr.nodes.size()) - 1;
        if (with_rest) top.kind = N_BIN, top.b = rest.root;
        else top.kind = N_SCAL, top.scalar = draw_scalar();
        s.expr.nodes.push_back(top);
        s.expr.root = static_cast<int>(s.expr.nodes.size()) - 1, s.expr.operators = with_rest ? rest.operators + 1 : 1;
        if (!mostly_finite(model.eval(s.expr).v)) return false;
        s.kind = ASSIGN_SHIFTED, s.dest_form = e.dense() ? D_DENSE_BLOCK : D_STRIDED_BLOCK;
        classify(s, dst);
        model.store(dst, model.eval(s.expr));
        return true;
    }
    bool with_expr(Stmt<T> &s, int kind) {
        if (!draw_expr(s.expr, rng.chance(3, 4) ? base_ : model.pool[random_live()].shape, -1, nullptr)) return false;
        count_leaves(s.expr);
        s.kind = kind;
        return true;
    }
    bool sum(Stmt<T> &s) {
        if (!draw_expr(s.expr, rng.chance(3, 4) ? base_ : model.pool[random_live()].shape, -1, nullptr)) return false;
        const Dense<T> d = model.eval(s.expr);
        for (T x : d.v) s.expect_sum += static_cast<long double>(x), s.sum_abs += std::fabs(static_cast<long double>(x));
        s.sum_n = d.v.size();
        if (!kFloat && s.sum_abs >= 9007199254740992.0L) return false;  // an integer sum must be exact in a double
        if (kFloat && !std::isfinite(static_cast<double>(s.sum_abs))) return false;
        count_leaves(s.expr);
        s.kind = rng.chance(1, 2) ? SUM_MEMBER : SUM_FREE;
        return true;
    }
    bool host_write(Stmt<T> &s) {
        const int slot = random_live_preferring_views();
        const View &e = model.pool[slot];
        std::vector<T> &st = model.storages[e.storage];
        const bool whole = e.offset == 0 && e.dense() && e.size() == st.size();
        s.slot = slot, s.dest_form = whole ? D_WHOLE : D_VIEW_ENTRY;
        const std::size_t r = rng.below(3), room = st.size() - e.offset;
        if (r == 0) {  // x.data[i] = v: positions from the entry's first element on, in the storage's own order
            s.kind = WRITE_DATA;
            for (std::size_t n = rng.range(1, 4); n-- > 0;) s.at.push_back(rng.below(room)), s.values.push_back(draw_value());
            for (std::size_t i = 0; i < s.values.size(); ++i) st[e.offset + s.at[i]] = s.values[i];
        } else if (r == 1) {  // x(i, j) = v through T&
            s.kind = WRITE_REF;
            for (std::size_t n = rng.range(1, 4); n-- > 0;) {
                std::size_t off = e.offset;
                for (std::size_t d = 0; d < e.shape.size(); ++d) s.at.push_back(rng.below(e.shape[d])), off += s.at.back() * e.strides[d];
                s.values.push_back(draw_value());
                st[off] = s.values.back();
            }
        } else {  // a loop through static_cast<T *>(x.data)
            s.kind = WRITE_BULK;
            const std::size_t first = rng.below(room), n = rng.range(1, room - first);
            s.at = {0, first}, s.values = draw_values(n);
            for (std::size_t i = 0; i < n; ++i) st[e.offset + first + i] = s.values[i];
        }
        return true;
    }
    bool host_read(Stmt<T> &s) {
        const int slot = random_live();
        const View &e = model.pool[slot];
        const std::vector<T> &st = model.storages[e.storage];
        s.slot = slot, s.dst.slot = slot;
        const std::size_t r = rng.below(8);
        if (r < 5) {  // bursts of 1 - 12 element reads: past the 8 after which the whole array is mirrored
            s.kind = READ_BURST;
            for (std::size_t n = rng.range(1, 12); n-- > 0;) {
                std::size_t off = e.offset;
                for (std::size_t d = 0; d < e.shape.size(); ++d) s.at.push_back(rng.below(e.shape[d])), off += s.at.back() * e.strides[d];
                s.expect.push_back(st[off]);
            }
        } else if (r < 7) {
            s.kind = READ_CDATA;
            s.expect = model.read(e).v, s.expect_shape = e.shape;
        } else {  // called, not compared: one row of anything large
            s.kind = TO_STRING;
            if (e.size() > 4096) {
                if (e.shape.size() < 2 || e.size() / e.shape[0] > 4096) return false;
                s.dst.sl.assign(e.shape.size(), Sl{});
                s.dst.sl[0] = Sl{2, rng.below(e.shape[0]), 0, 1};
            }
        }
        return true;
    }
    bool assign_where(Stmt<T> &s) {
        if (!draw_destination(s)) return false;
        const View dst = model.view(s.dst);
        s.kind = ASSIGN_WHERE, s.scalar = draw_scalar(), s.scalar2 = draw_value();
        if (!is_finite(s.scalar2)) s.scalar2 = T(1);
        T *base = model.storages[dst.storage].data() + dst.offset;
        walk(dst.shape, dst.strides, dst.strides, [&](std::size_t, std::size_t o, std::size_t) {
            if (base[o] > s.scalar) base[o] = s.scalar2;
        });
        return true;
    }
    bool put_along_axis(Stmt<T> &s) {
        if (!draw_destination(s)) return false;
        const View dst = model.view(s.dst);
        const std::size_t nd = dst.shape.size();
        s.kind = PUT_ALONG_AXIS, s.axis = static_cast<int>(rng.below(nd)), s.scalar = draw_value();
        if (!is_finite(s.scalar)) s.scalar = T(1);
        const std::size_t extent = dst.shape[s.axis];
        s.index_shape = dst.shape;
        s.index_shape[s.axis] = rng.range(1, extent < 3 ? extent : 3);
        for (std::size_t d = 0; d < nd; ++d)
            if (static_cast<int>(d) != s.axis && rng.chance(1, 3)) s.index_shape[d] = 1;  // broadcast against the target
        s.index.resize(prod(s.index_shape));
        for (std::int64_t &i : s.index) i = static_cast<std::int64_t>(rng.below(2 * extent)) - static_cast<std::int64_t>(extent);  // [-R, R): negatives count from the end
        // the walk: the target's shape with the index's extent on the axis
        Shape walk_shape = dst.shape;
        walk_shape[s.axis] = s.index_shape[s.axis];
        Shape sd = dst.strides;
        sd[s.axis] = 0;
        const Shape si = strides_over(s.index_shape, dense_strides(s.index_shape), walk_shape);
        T *base = model.storages[dst.storage].data() + dst.offset;
        walk(walk_shape, sd, si, [&](std::size_t, std::size_t o, std::size_t oi) {
            const std::int64_t i = s.index[oi] < 0 ? s.index[oi] + static_cast<std::int64_t>(extent) : s.index[oi];
            base[o + static_cast<std::size_t>(i) * dst.strides[s.axis]] = s.scalar;
        });
        return true;
    }

    // ---- families fed a pending chain or a view; the order is sort's: a before b when a < b, or b is a NaN and a is not
    static bool before(T a, T b) { return a < b || (is_nan(b) && !is_nan(a)); }
    bool family(Stmt<T> &s) {
        Dense<T> d;
        if (rng.chance(1, 3)) {  // a view, read in place
            const int slot = random_live();
            if (!make_spec(slot, static_cast<int>(rng.below(7)), model.pool[slot].shape, false, s.dst)) return false;
            s.fed_view = true, s.slot = slot;
            d = model.read(model.view(s.dst));
        } else {
            if (!draw_expr(s.expr, rng.chance(3, 4) ? base_ : model.pool[random_live()].shape, -1, nullptr)) return false;
            count_leaves(s.expr);
            d = model.eval(s.expr);
        }
        if (d.v.empty() || d.shape.empty()) return false;
        const std::size_t nd = d.shape.size();
        s.kind = FAMILY_MAX + static_cast<int>(rng.below(4));
        s.axis = static_cast<int>(rng.below(nd));
        const std::size_t n = d.shape[s.axis];
        if (s.kind == FAMILY_SORT && n > 2048) return false;  // the model's sort is quadratic
        std::size_t inner = 1;
        for (std::size_t i = s.axis + 1; i < nd; ++i) inner *= d.shape[i];
        const std::size_t outer = d.v.size() / (n * inner);
        const bool reduces = s.kind == FAMILY_MAX || s.kind == FAMILY_ARGMAX;
        s.expect_shape = d.shape;
        if (reduces) {
            s.expect_shape.erase(s.expect_shape.begin() + s.axis);
            if (s.expect_shape.empty()) s.expect_shape = {1};
        }
        if (s.kind == FAMILY_ARGMAX) s.expect_index.resize(outer * inner);
        else s.expect.resize(reduces ? outer * inner : d.v.size());
        s.zero_ties_free = s.kind == FAMILY_MAX || s.kind == FAMILY_CUMMAX;
        std::vector<T> line(n);
        for (std::size_t o = 0; o < outer; ++o)
            for (std::size_t in = 0; in < inner; ++in) {
                const T *p = d.v.data() + o * n * inner + in;
                for (std::size_t i = 0; i < n; ++i) line[i] = p[i * inner];
                if (reduces) {  // the first NaN if there is one, else the first of the largest
                    std::size_t best = 0;
                    for (std::size_t i = 1; i < n && !is_nan(line[best]); ++i)
                        if (is_nan(line[i]) || line[i] > line[best]) best = i;
                    if (s.kind == FAMILY_MAX) s.expect[o * inner + in] = line[best];
                    else s.expect_index[o * inner + in] = static_cast<std::int64_t>(best);
                } else if (s.kind == FAMILY_CUMMAX) {  // from a NaN on, NaN
                    T run = line[0];
                    for (std::size_t i = 0; i < n; ++i) {
                        if (!is_nan(run) && (is_nan(line[i]) || line[i] > run)) run = line[i];
                        s.expect[(o * n + i) * inner + in] = run;
                    }
                } else {  // stable, ascending, NaNs last: an insertion sort of the line (the operand's own bits)
                    for (std::size_t i = 1; i < n; ++i) {
                        const T x = line[i];
                        std::size_t j = i;
                        for (; j > 0 && before(x, line[j - 1]); --j) line[j] = line[j - 1];
                        line[j] = x;
                    }
                    for (std::size_t i = 0; i < n; ++i) s.expect[(o * n + i) * inner + in] = line[i];
                }
            }
        return true;
    }

    bool drop(Stmt<T> &s) {
        const int slot = random_live();
        if (slot < 0 || model.live_count() <= 4) return false;
        const View &e = model.pool[slot];
        if (e.offset == 0 && e.size() == model.storages[e.storage].size() && model.users(e.storage) > 1) cov_.tick("drop  an owner while a view lives");
        s.kind = DROP, s.slot = slot;
        model.release(slot);
        return true;
    }
    bool move(Stmt<T> &s) {
        int from = random_live();
        const int to = model.free_slot();
        for (int attempt = 0; attempt < 4 && from >= 0 && model.pool[from].dense() && model.pool[from].offset == 0; ++attempt) from = random_live();  // a view, by preference
        if (from < 0 || to < 0) return false;
        const View &e = model.pool[from];
        if (!(e.offset == 0 && e.dense() && e.size() == model.storages[e.storage].size())) cov_.tick("move  of a view");
        s.kind = MOVE, s.slot = from, s.slot2 = to, s.dest_form = D_NEW;
        model.pool[to] = model.pool[from];
        model.pool[from] = View{};
        return true;
    }
    bool contiguous(Stmt<T> &s) {
        const int from = random_live(), to = model.free_slot();
        if (from < 0 || to < 0) return false;
        if (!make_spec(from, static_cast<int>(rng.below(7)), model.pool[from].shape, false, s.dst)) return false;
        s.kind = CONTIGUOUS, s.slot = from, s.slot2 = to, s.dest_form = D_NEW;
        Dense<T> d = model.read(model.view(s.dst));
        model.birth(to, d.shape, std::move(d.v));
        return true;
    }
    bool repeat(Stmt<T> &s) {  // numpy's: every element `repeats` times, flattened; observed, not kept
        const int from = random_live();
        if (!make_spec(from, static_cast<int>(rng.below(7)), model.pool[from].shape, false, s.dst)) return false;
        const Dense<T> d = model.read(model.view(s.dst));
        s.kind = REPEAT, s.slot = from, s.repeats = static_cast<int>(rng.range(1, 3));
        if (d.v.size() * s.repeats > (std::size_t{1} << 20)) return false;
        for (T x : d.v)
            for (int k = 0; k < s.repeats; ++k) s.expect.push_back(x);
        s.expect_shape = {s.expect.size()};
        return true;
    }
    // auto r = E op (a write to one of E's operands, y): the write comes while E's chain is pending and must not reach E
    bool write_mid(Stmt<T> &s) {
        const int to = model.free_slot();
        if (to < 0 || !draw_expr(s.expr, base_, -1, nullptr)) return false;
        std::vector<int> slots;
        for (const Node<T> &n : s.expr.nodes)
            if (n.kind == N_LEAF) slots.push_back(n.leaf.slot);
        if (!draw_leaf(base_, false, model.pool[slots[rng.below(slots.size())]].storage, s.dst)) return false;
        const Dense<T> left = model.eval(s.expr);
        s.kind = WRITE_MID, s.slot = slots[rng.below(slots.size())], s.slot2 = to, s.dest_form = D_NEW, s.op = static_cast<int>(rng.below(3)), s.variant = static_cast<int>(rng.below(2));
        const View &x = model.pool[s.slot];
        std::vector<T> &st = model.storages[x.storage];
        if (s.variant == 0) {
            for (std::size_t n = rng.range(1, 6); n-- > 0;) s.at.push_back(rng.below(st.size() - x.offset)), s.values.push_back(draw_value());
            for (std::size_t i = 0; i < s.values.size(); ++i) st[x.offset + s.at[i]] = s.values[i];
        } else {
            s.scalar = draw_scalar(), s.scalar2 = draw_scalar();
            T *base = st.data() + x.offset;
            walk(x.shape, x.strides, x.strides, [&](std::size_t, std::size_t o, std::size_t) {
                if (base[o] > s.scalar) base[o] = s.scalar2;
            });
        }
        Dense<T> r = model.binary(s.op, left, model.read(model.view(s.dst)));
        count_leaves(s.expr);
        model.birth(to, r.shape, std::move(r.v));
        return true;
    }
    // a statement that throws: the pool must equal the model afterwards
    bool refused(Stmt<T> &s) {
        if (rng.chance(1, 2)) {  // E + w, w of a shape that does not broadcast: thrown while E's chain is pending
            Expr<T> e;
            if (!draw_expr(e, base_, -1, nullptr, 2)) return false;
            ViewSpec wrong;
            bool found = false;
            for (int attempt = 0; attempt < 20 && !found; ++attempt) {
                wrong = ViewSpec{};
                wrong.slot = random_live();
                Shape out;
                found = !broadcast(base_, model.pool[wrong.slot].shape, out);
            }
            if (!found) return false;
            Node<T> leaf, top;
            leaf.leaf = wrong;
            e.nodes.push_back(leaf);
            top.kind = N_BIN, top.op = static_cast<int>(rng.below(4)), top.a = e.root, top.b = static_cast<int>(e.nodes.size()) - 1;
            e.nodes.push_back(top);
            e.root = static_cast<int>(e.nodes.size()) - 1;
            s.expr = e, s.kind = REFUSED_EXPR;
        } else {  // x(row) = E of the whole shape
            const int slot = random_live();
            const View &e = model.pool[slot];
            if (e.shape.size() < 2 || e.shape[0] < 2) return false;
            if (!draw_expr(s.expr, e.shape, e.storage, nullptr)) return false;
            s.slot = slot, s.dst.slot = slot;
            s.dst.sl.assign(e.shape.size(), Sl{});
            s.dst.sl[0] = Sl{2, rng.below(e.shape[0]), 0, 1};
            s.kind = REFUSED_ROW, s.dest_form = D_ROW;
        }
        return true;
    }
};

}  // namespace sfm

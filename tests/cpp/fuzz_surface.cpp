// fuzz_surface.cpp -- the model-based fuzzer of the C++ surface: random programs over a pool of named sm::SMArray<T> (float, double,
// int, std::int64_t), executed through include/sm.h on the GPU and on the host model of tests/cpp/surface_model.h, every observation
// compared: arrays bit for bit (a NaN on both sides counts as equal), float sums within the bound of any fp64 summation order, integer
// sums exactly.  What it walks is the state the header carries: Storage's validity bits and fetch counter, `data` and T& as writable
// handles, the one pending chain per thread and its flush before writes, direct assignment (Chain::may_write_into), chain cutting,
// and the tiny-operator recorder and the two queues behind them.
//
//   fuzz_surface [--seed S] [--cases N] [--case K] [--class tiny|small|mid]
//
// An expression tree is evaluated as the statement it stands for: every operator argument binds to the same detail::Operand /
// detail::ScalarArg wrapper the compiler would create, and they die together, last made first, at the end of the statement (Frame) --
// so a chain stays pending across the operators of one statement and is launched where `;` would launch it.
// On a mismatch: seed, case, first differing element, both values, the case's statements as text; the case ends; the exit status is 1.
// An exception nobody expected (a library call that failed) ends the run at once with exit status 3.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <memory>
#include <utility>

#include "sm.h"
#include "surface_model.h"

using sm::SMArray;
using namespace sfm;

namespace {

struct Totals {
    std::uint64_t hash = 0xcbf29ce484222325ull;
    unsigned long long compared = 0, mismatches = 0, cases = 0;
    bool stopped = false;  // an exception nobody expected (a failed library call): nothing more is started on the device
    void feed(const void *p, std::size_t n) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (std::size_t i = 0; i < n; ++i) hash = (hash ^ b[i]) * 0x100000001b3ull;
        compared += n;
    }
};

struct Mismatch {
    std::string what;
};

template <typename T> Slice slice_of(const Sl &s) {
    if (s.kind == 2) return Slice::index(s.a);
    if (s.kind == 0) return Slice(0);
    Slice r(s.a, s.b);
    if (s.step > 1) r.step = static_cast<Slice::SliceStep>(s.step);
    return r;
}

template <typename T> class Runner {
public:
    Runner(std::uint64_t seed, std::uint64_t k, Totals &totals) : seed_(seed), case_(k), totals_(totals) {}

    bool run(Coverage &cov) {
        Case<T> c(seed_, k_case(), cov);
        Stmt<T> s;
        try {
            while (c.next(s)) {
                text_.push_back(text_of(s));
                exec(s, c.model);
            }
        } catch (const Mismatch &m) {
            report(m.what);
            return false;
        } catch (const std::exception &e) {
            report(std::string("unexpected exception: ") + e.what());
            totals_.stopped = true;
            return false;
        }
        return true;
    }

private:
    using Operand = sm::detail::Operand<T>;
    using ScalarArg = sm::detail::ScalarArg<T>;
    std::uint64_t seed_, case_;
    Totals &totals_;
    std::unique_ptr<SMArray<T>> pool_[Model<T>::kSlots];
    std::vector<std::string> text_;
    std::uint64_t k_case() const { return case_; }

    void report(const std::string &what) {
        ++totals_.mismatches;
        std::printf("MISMATCH seed %llu case %llu (%s, %s): %s\n", static_cast<unsigned long long>(seed_), static_cast<unsigned long long>(case_),
                    type_info_of<T>::name, class_name(class_of_case(case_)), what.c_str());
        for (std::size_t i = 0; i < text_.size(); ++i) std::printf("  [%zu] %s\n", i, text_[i].c_str());
        std::fflush(stdout);
    }
    [[noreturn]] void fail(const std::string &where, std::size_t index, T want, T got) {
        throw Mismatch{where + ": element " + std::to_string(index) + ": model " + num_text(want) + " (bits " + std::to_string(bits_of(want)) + "), device " + num_text(got) +
                       " (bits " + std::to_string(bits_of(got)) + ")"};
    }

    // The temporaries of one statement: results, views and the operators' argument wrappers, destroyed last made first.
    struct Frame {
        struct Item {
            std::unique_ptr<SMArray<T>> arr;
            std::unique_ptr<Operand> op;
            std::unique_ptr<ScalarArg> sc;
        };
        std::vector<Item> items;
        SMArray<T> *hold(SMArray<T> &&a) {
            items.emplace_back();
            items.back().arr = std::make_unique<SMArray<T>>(std::move(a));
            return items.back().arr.get();
        }
        const Operand &operand(SMArray<T> *p, bool temporary) {
            items.emplace_back();
            items.back().op.reset(temporary ? new Operand(std::move(*p)) : new Operand(static_cast<const SMArray<T> &>(*p)));
            return *items.back().op;
        }
        const ScalarArg &scalar(T v) {
            items.emplace_back();
            items.back().sc.reset(new ScalarArg(v));
            return *items.back().sc;
        }
        ~Frame() noexcept(false) {
            while (!items.empty()) items.pop_back();
        }
    };
    struct Val {
        SMArray<T> *p;
        bool temporary;
    };

    static SMArray<T> subscript(const SMArray<T> &a, const std::vector<Sl> &sl) {
        const auto S = [&](std::size_t d) { return slice_of<T>(sl[d]); };
        switch (sl.size()) {
            case 1: return a(S(0));
            case 2: return a(S(0), S(1));
            case 3: return a(S(0), S(1), S(2));
            default: return a(S(0), S(1), S(2), S(3));
        }
    }
    bool whole(const ViewSpec &sp) const { return !sp.transpose && sp.sl.empty(); }
    SMArray<T> view(const ViewSpec &sp) const {  // not for whole(sp): an entry itself is an lvalue
        const SMArray<T> &base = *pool_[sp.slot];
        if (!sp.transpose) return subscript(base, sp.sl);
        if (sp.sl.empty()) return base.transpose();
        return subscript(base.transpose(), sp.sl);
    }
    Val place(const ViewSpec &sp, Frame &f) {
        if (whole(sp)) return Val{pool_[sp.slot].get(), false};
        return Val{f.hold(view(sp)), true};
    }

    static SMArray<T> binary(int op, Val a, const Operand &b) {
        if (a.temporary) {
            switch (op) {
                case 0: return std::move(*a.p) + b;
                case 1: return std::move(*a.p) - b;
                case 2: return std::move(*a.p) * b;
                default: return std::move(*a.p) / b;
            }
        }
        switch (op) {
            case 0: return *a.p + b;
            case 1: return *a.p - b;
            case 2: return *a.p * b;
            default: return *a.p / b;
        }
    }
    static SMArray<T> binary(int op, Val a, const ScalarArg &b) {
        if (a.temporary) {
            switch (op) {
                case 0: return std::move(*a.p) + b;
                case 1: return std::move(*a.p) - b;
                case 2: return std::move(*a.p) * b;
                default: return std::move(*a.p) / b;
            }
        }
        switch (op) {
            case 0: return *a.p + b;
            case 1: return *a.p - b;
            case 2: return *a.p * b;
            default: return *a.p / b;
        }
    }
    Val eval(const Expr<T> &e, int at, Frame &f) {
        const Node<T> &n = e.nodes[at];
        switch (n.kind) {
            case N_LEAF: return place(n.leaf, f);
            case N_BIN: {
                const Val a = eval(e, n.a, f), b = eval(e, n.b, f);
                const Operand &rhs = f.operand(b.p, b.temporary);
                return Val{f.hold(binary(n.op, a, rhs)), true};
            }
            case N_SCAL: {
                const Val a = eval(e, n.a, f);
                const ScalarArg &rhs = f.scalar(n.scalar);
                return Val{f.hold(binary(n.op, a, rhs)), true};
            }
            case N_LSCAL: {
                const Val one{f.hold(SMArray<T>{n.scalar}), true};
                const Val a = eval(e, n.a, f);
                const Operand &rhs = f.operand(a.p, a.temporary);
                return Val{f.hold(binary(n.op, one, rhs)), true};
            }
            case N_NEG: {
                const Val a = eval(e, n.a, f);
                return Val{f.hold(a.temporary ? -std::move(*a.p) : -*a.p), true};
            }
            case N_ABS: {
                const Val a = eval(e, n.a, f);
                return Val{f.hold(a.temporary ? sm::abs(std::move(*a.p)) : sm::abs(*a.p)), true};
            }
            case N_SQRTABS: {
                const Val a = eval(e, n.a, f);
                if constexpr (std::is_floating_point_v<T>) {
                    SMArray<T> *t = f.hold(a.temporary ? sm::abs(std::move(*a.p)) : sm::abs(*a.p));
                    return Val{f.hold(sm::sqrt(std::move(*t))), true};
                } else {
                    return a;
                }
            }
            default: {
                const Val a = eval(e, n.a, f);
                if constexpr (!std::is_floating_point_v<T>) return Val{f.hold(a.temporary ? sm::pow(std::move(*a.p), static_cast<T>(n.k)) : sm::pow(*a.p, static_cast<T>(n.k))), true};
                else return a;
            }
        }
    }
    Val eval(const Expr<T> &e, Frame &f) { return eval(e, e.root, f); }

    static SMArray<T> ones_or_zeros(bool ones, const Shape &s) {
        switch (s.size()) {
            case 1: return ones ? sm::ones<T>(s[0]) : sm::zeros<T>(s[0]);
            case 2: return ones ? sm::ones<T>(s[0], s[1]) : sm::zeros<T>(s[0], s[1]);
            case 3: return ones ? sm::ones<T>(s[0], s[1], s[2]) : sm::zeros<T>(s[0], s[1], s[2]);
            default: return ones ? sm::ones<T>(s[0], s[1], s[2], s[3]) : sm::zeros<T>(s[0], s[1], s[2], s[3]);
        }
    }
    static SMArray<T> list_of(const std::vector<T> &v, const Shape &shape) {
        if (shape.size() == 2) return SMArray<T>{{v[0], v[1], v[2]}, {v[3], v[4], v[5]}};
        switch (v.size()) {
            case 1: return SMArray<T>{v[0]};
            case 2: return SMArray<T>{v[0], v[1]};
            case 3: return SMArray<T>{v[0], v[1], v[2]};
            case 4: return SMArray<T>{v[0], v[1], v[2], v[3]};
            case 5: return SMArray<T>{v[0], v[1], v[2], v[3], v[4]};
            default: return SMArray<T>{v[0], v[1], v[2], v[3], v[4], v[5]};
        }
    }
    static SMArray<T> adopted(const std::vector<T> &v, const Shape &shape) {
        T *buffer = new T[v.size() ? v.size() : 1];
        std::copy(v.begin(), v.end(), buffer);
        return SMArray<T>(buffer, Shape(shape));
    }
    static T &element(SMArray<T> &a, const std::size_t *i) {
        switch (a.shape().size()) {
            case 1: return a(i[0]);
            case 2: return a(i[0], i[1]);
            case 3: return a(i[0], i[1], i[2]);
            default: return a(i[0], i[1], i[2], i[3]);
        }
    }
    static T element(const SMArray<T> &a, const std::size_t *i) {
        switch (a.shape().size()) {
            case 1: return a(i[0]);
            case 2: return a(i[0], i[1]);
            case 3: return a(i[0], i[1], i[2]);
            default: return a(i[0], i[1], i[2], i[3]);
        }
    }

    // the elements of `a` in row-major order against `want`
    template <typename U> void compare(const std::string &where, const SMArray<U> &a, const Shape &shape, const std::vector<U> &want, bool zero_ties_free = false) {
        if (a.shape() != shape) throw Mismatch{where + ": shape " + text_of(a.shape()) + ", the model has " + text_of(shape)};
        const U *base = a.cdata();
        std::size_t bad = want.size();
        walk(shape, a.strides(), a.strides(), [&](std::size_t lin, std::size_t o, std::size_t) {
            const U got = base[o];
            totals_.feed(&got, sizeof got);
            if (bad == want.size() && !same_bits(want[lin], got) && !(zero_ties_free && want[lin] == 0 && got == 0)) bad = lin;
        });
        if (bad != want.size()) {
            U got{};
            walk(shape, a.strides(), a.strides(), [&](std::size_t lin, std::size_t o, std::size_t) { if (lin == bad) got = base[o]; });
            throw Mismatch{where + ": element " + std::to_string(bad) + ": model " + num_text(want[bad]) + " (bits " + std::to_string(bits_of(want[bad])) + "), device " +
                           num_text(got) + " (bits " + std::to_string(bits_of(got)) + ")"};
        }
    }

    void exec(const Stmt<T> &s, const Model<T> &model) {
        switch (s.kind) {
            case BIRTH_ONES: pool_[s.slot2] = std::make_unique<SMArray<T>>(ones_or_zeros(true, s.shape) * s.scalar); break;
            case BIRTH_ZEROS: pool_[s.slot2] = std::make_unique<SMArray<T>>(ones_or_zeros(false, s.shape) * s.scalar); break;
            case BIRTH_LIST: pool_[s.slot2] = std::make_unique<SMArray<T>>(list_of(s.values, s.shape)); break;
            case BIRTH_ADOPT: case BIRTH_HOST_TINY: case BIRTH_HOST_SMALL: pool_[s.slot2] = std::make_unique<SMArray<T>>(adopted(s.values, s.shape)); break;
            case VIEW_NEW: pool_[s.slot2] = std::make_unique<SMArray<T>>(view(s.dst)); break;
            case EXPR_NEW: {
                Frame f;
                const Val v = eval(s.expr, f);
                pool_[s.slot2] = std::make_unique<SMArray<T>>(std::move(*v.p));
                break;
            }
            case ASSIGN: case ASSIGN_SHIFTED: {
                Frame f;
                const Val v = eval(s.expr, f);
                const Val d = place(s.dst, f);
                *d.p = std::move(*v.p);
                break;
            }
            case ASSIGN_TRANSPOSE: *pool_[s.slot] = pool_[s.slot]->transpose(); break;
            case DISCARD: {
                Frame f;
                (void)eval(s.expr, f);
                break;
            }
            case REFUSED_EXPR: case REFUSED_ROW: {
                bool threw = false;
                try {
                    Frame f;
                    const Val v = eval(s.expr, f);
                    if (s.kind == REFUSED_ROW) {
                        const Val d = place(s.dst, f);
                        *d.p = std::move(*v.p);
                    }
                } catch (const Mismatch &) {
                    throw;
                } catch (const std::exception &) {
                    threw = true;
                }
                if (!threw) throw Mismatch{"the statement was not refused"};
                break;
            }
            case SUM_MEMBER: case SUM_FREE: {
                double got;
                {
                    Frame f;
                    const Val v = eval(s.expr, f);
                    got = s.kind == SUM_MEMBER ? std::move(*v.p).sum() : sm::sum(std::move(*v.p));
                }
                totals_.feed(&got, sizeof got);
                // any fp64 summation order: (n - 1) 2^-53 sum|x|, and the final rounding to double; integers (sum|x| < 2^53) exactly
                const long double allowed = std::is_floating_point_v<T> ? (static_cast<long double>(s.sum_n ? s.sum_n - 1 : 0) * s.sum_abs + std::fabs(s.expect_sum)) * 0x1p-53L : 0.0L;
                const long double off = std::fabs(static_cast<long double>(got) - s.expect_sum);
                if (!(off <= allowed)) throw Mismatch{"sum: model " + num_text(static_cast<double>(s.expect_sum)) + ", device " + num_text(got) + ", allowed " + num_text(static_cast<double>(allowed))};
                break;
            }
            case WRITE_DATA:
                for (std::size_t i = 0; i < s.values.size(); ++i) pool_[s.slot]->data[s.at[i]] = s.values[i];
                break;
            case WRITE_REF: {
                const std::size_t nd = pool_[s.slot]->shape().size();
                for (std::size_t i = 0; i < s.values.size(); ++i) element(*pool_[s.slot], s.at.data() + i * nd) = s.values[i];
                break;
            }
            case WRITE_BULK: case RESEED: {
                T *p = static_cast<T *>(pool_[s.slot]->data) - s.at[0];
                for (std::size_t i = 0; i < s.values.size(); ++i) p[s.at[1] + i] = s.values[i];
                break;
            }
            case READ_BURST: {
                const std::size_t nd = pool_[s.slot]->shape().size();
                for (std::size_t i = 0; i < s.expect.size(); ++i) {
                    const T got = element(std::as_const(*pool_[s.slot]), s.at.data() + i * nd);
                    totals_.feed(&got, sizeof got);
                    if (!same_bits(s.expect[i], got)) fail("as_const(v" + std::to_string(s.slot) + ")(...) read " + std::to_string(i), i, s.expect[i], got);
                }
                break;
            }
            case READ_CDATA: compare("cdata() of v" + std::to_string(s.slot), *pool_[s.slot], s.expect_shape, s.expect); break;
            case TO_STRING: {
                Frame f;
                (void)place(s.dst, f).p->toString();
                break;
            }
            case ASSIGN_WHERE: {
                Frame f;
                SMArray<T> &x = *place(s.dst, f).p;
                x.assign_where(x > s.scalar, s.scalar2);
                break;
            }
            case PUT_ALONG_AXIS: {
                std::int64_t *buffer = new std::int64_t[s.index.size()];
                std::copy(s.index.begin(), s.index.end(), buffer);
                const SMArray<std::int64_t> idx(buffer, Shape(s.index_shape));
                Frame f;
                place(s.dst, f).p->put_along_axis(idx, s.scalar, s.axis);
                break;
            }
            case FAMILY_MAX: case FAMILY_ARGMAX: case FAMILY_SORT: case FAMILY_CUMMAX: {
                Frame f;
                const Val v = s.fed_view ? place(s.dst, f) : eval(s.expr, f);
                const std::string where = kind_name(s.kind);
                if (s.kind == FAMILY_ARGMAX) compare(where, sm::argmax(*v.p, s.axis), s.expect_shape, s.expect_index);
                else if (s.kind == FAMILY_MAX) compare(where, sm::max(*v.p, s.axis), s.expect_shape, s.expect, true);
                else if (s.kind == FAMILY_SORT) compare(where, sm::sort(*v.p, s.axis), s.expect_shape, s.expect);
                else compare(where, sm::cummax(*v.p, s.axis), s.expect_shape, s.expect, true);
                break;
            }
            case DROP: pool_[s.slot].reset(); break;
            case DROP_RESULT: {
                std::unique_ptr<SMArray<T>> r;
                {
                    Frame f;
                    const Val v = eval(s.expr, f);
                    r = std::make_unique<SMArray<T>>(std::move(*v.p));
                }
                r.reset();
                break;
            }
            case MOVE: {
                SMArray<T> y = std::move(*pool_[s.slot]);
                pool_[s.slot].reset();
                pool_[s.slot2] = std::make_unique<SMArray<T>>(std::move(y));
                break;
            }
            case CONTIGUOUS: {
                Frame f;
                pool_[s.slot2] = std::make_unique<SMArray<T>>(place(s.dst, f).p->contiguous());
                break;
            }
            case REPEAT: {
                Frame f;
                compare("repeat", place(s.dst, f).p->repeat(s.repeats), s.expect_shape, s.expect);
                break;
            }
            case WRITE_MID: {
                Frame f;
                const Val left = eval(s.expr, f);  // pending from here on
                SMArray<T> &x = *pool_[s.slot];
                if (s.variant == 0) {
                    for (std::size_t i = 0; i < s.values.size(); ++i) x.data[s.at[i]] = s.values[i];
                } else {
                    x.assign_where(x > s.scalar, s.scalar2);
                }
                const Val y = place(s.dst, f);
                const Operand &rhs = f.operand(y.p, y.temporary);
                pool_[s.slot2] = std::make_unique<SMArray<T>>(binary(s.op, left, rhs));
                break;
            }
            default:  // COMPARE: the whole pool against the model
                for (int i = 0; i < Model<T>::kSlots; ++i) {
                    const View &m = model.pool[i];
                    if (m.live() != static_cast<bool>(pool_[i])) throw Mismatch{"v" + std::to_string(i) + " lives on one side only"};
                    if (m.live()) compare("v" + std::to_string(i), *pool_[i], m.shape, model.read(m).v);
                }
                break;
        }
    }
};

template <typename T> bool run_case(std::uint64_t seed, std::uint64_t k, Totals &totals, Coverage &cov) {
    Runner<T> r(seed, k, totals);
    return r.run(cov);
}

}  // namespace

int main(int argc, char **argv) {
    std::uint64_t seed = 1, cases = 40;
    long long only = -1;
    int only_class = -1;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        const char *v = i + 1 < argc ? argv[i + 1] : "";
        if (a == "--seed") seed = std::strtoull(v, nullptr, 10), ++i;
        else if (a == "--cases") cases = std::strtoull(v, nullptr, 10), ++i;
        else if (a == "--case") only = std::atoll(v), ++i;
        else if (a == "--class") only_class = std::string(v) == "tiny" ? TINY : std::string(v) == "small" ? SMALL : MID, ++i;
        else {
            std::fprintf(stderr, "usage: fuzz_surface [--seed S] [--cases N] [--case K] [--class tiny|small|mid]\n");
            return 2;
        }
    }
    Totals totals;
    Coverage cov;
    for (std::uint64_t k = only >= 0 ? static_cast<std::uint64_t>(only) : 0; k < (only >= 0 ? static_cast<std::uint64_t>(only) + 1 : cases); ++k) {
        if (only_class >= 0 && class_of_case(k) != only_class) continue;
        if (totals.stopped) break;
        ++totals.cases;
        switch (type_of_case(k)) {
            case 0: run_case<float>(seed, k, totals, cov); break;
            case 1: run_case<double>(seed, k, totals, cov); break;
            case 2: run_case<int>(seed, k, totals, cov); break;
            default: run_case<std::int64_t>(seed, k, totals, cov); break;
        }
    }
    if (totals.stopped) {
        std::printf("fuzz_surface seed %llu: stopped in case %llu of %llu by an unexpected exception\n", static_cast<unsigned long long>(seed), totals.cases - 1,
                    static_cast<unsigned long long>(cases));
        std::fflush(stdout);
        std::_Exit(3);  // no further call into the library, not even the destructors'
    }
    sm::synchronize();
    cov.print(std::cout);
    const auto fs = sm::fusion_stats();
    std::printf("fusion: chains %llu fused_stages %llu single_ops %llu direct_assignments %llu summed_chains %llu\n", fs.chains, fs.fused_stages, fs.single_ops,
                fs.direct_assignments, fs.summed_chains);
    unsigned long long launches = 0, operators = 0, alternations = 0, edges = 0;
    int queues = 0;
    smhip_tiny_stats(&launches, &operators);
    smhip_queue_stats(&queues, &alternations, &edges);
    std::printf("tiny: launches %llu operators %llu\n", launches, operators);
    std::printf("queues: %d alternations %llu edges %llu\n", queues, alternations, edges);
    std::printf("hash: %016llx over %llu bytes\n", static_cast<unsigned long long>(totals.hash), totals.compared);
    std::printf("fuzz_surface seed %llu: %llu cases, %llu mismatches\n", static_cast<unsigned long long>(seed), totals.cases, totals.mismatches);
    return totals.mismatches ? 1 : 0;
}

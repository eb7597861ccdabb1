// rmc_pred_compile.h — the compiler of model-defined invariants: a state predicate of the
// model's .tla, in the typed subset of TLA+ that rmc.h ("model-defined invariants") and
// DESIGN.md list, to the bytecode of rmc_pred.h.  Part of the front-end: included by
// rmc_front.cpp inside its unnamed namespace, after Tok, Unit and Ctx (it uses tokenize,
// Ctx::def, Ctx::int_of and kRaftUnits).  Host only.
//
// Two steps: a precedence parser over the definition's tokens (infix operators and
// column-aligned junction lists: a token at or left of a list's bullet column ends the
// item) builds a tree; the generator types it, expands references to the model's own
// definitions in place, and emits code while it tracks the stack depth, the bound names
// in scope and the code size — the bounds the interpreter relies on.  Whatever is not in
// the language is refused by name, with its line and column.
//
// An action property's body (PROPERTY [][A]_vars, compile_actions; DESIGN.md "Action
// properties") is the same language plus primes: the parser accepts x', (e)', Name' and
// Name(args)' as a PRIME node, and the generator emits the successor's state reads
// (OP_PRIMED) for a primed variable and for every read inside a primed expression.  A
// bound message remembers the bag it was bound in.  Without primes nothing changes.

struct PNode;
typedef std::shared_ptr<PNode> PNodeP;
struct PNode {
    enum Kind { NUM, ID, INDEX, CALL, FIELD, NOT, BIN, IF, QUANT, SETLIT, SETCOMP, DOMAIN, RANGE, PRIME } kind;
    std::string s;  // NUM: digits; ID / CALL / FIELD: the name; BIN: the operator; QUANT: \A or \E; SETCOMP: the bound name
    int line = 0, col = 0;
    std::vector<PNodeP> k;
    std::vector<std::string> names;  // QUANT: bound names, k = {domain per name..., body}
};

struct PredError {
    std::string msg;
};

inline std::string at_of(int line, int col) { return " at line " + std::to_string(line) + ", col " + std::to_string(col); }

class PredParser {
    const std::vector<Tok>& v;
    size_t i = 0;
    std::vector<int> margin;  // bullet columns of the open junction lists
    bool primes;              // an action property's body: x', (e)', Name', Name(args)' are accepted

    const Tok* peek() const {
        if (i >= v.size()) return nullptr;
        if (!margin.empty() && v[i].col <= margin.back()) return nullptr;
        return &v[i];
    }
    bool is(const char* t) const {
        const Tok* p = peek();
        return p && p->t == t;
    }
    bool is_any(std::initializer_list<const char*> ts) const {
        for (const char* t : ts)
            if (is(t)) return true;
        return false;
    }
    [[noreturn]] void refuse(const std::string& what, const Tok* p) const {
        if (p) throw PredError{what + at_of(p->line, p->col)};
        const Tok& l = v[v.size() ? std::min(i, v.size() - 1) : 0];
        throw PredError{what + " after line " + std::to_string(l.line) + ", col " + std::to_string(l.col)};
    }
    Tok expect(const char* t) {
        const Tok* p = peek();
        if (!p || p->t != t) refuse(std::string("expected `") + t + "`" + (p ? ", found `" + p->t + "`" : ""), p);
        return v[i++];
    }
    static PNodeP node(PNode::Kind k, const Tok& t, const std::string& s = "") {
        PNodeP n = std::make_shared<PNode>();
        n->kind = k;
        n->s = s;
        n->line = t.line;
        n->col = t.col;
        return n;
    }
    static PNodeP bin(const Tok& op, const std::string& name, PNodeP a, PNodeP b) {
        PNodeP n = node(PNode::BIN, op, name);
        n->k = {a, b};
        return n;
    }
    static bool ident_tok(const std::string& t) { return !t.empty() && (isalpha((unsigned char)t[0]) || t[0] == '_'); }

public:
    explicit PredParser(const std::vector<Tok>& toks, bool accept_primes = false) : v(toks), primes(accept_primes) {}

    PNodeP parse_all() {
        if (v.empty()) throw PredError{"the definition is empty"};
        PNodeP n = expr();
        if (i < v.size()) refuse("unexpected `" + v[i].t + "`", &v[i]);
        return n;
    }

    // TLA+'s levels: => (1) binds looser than <=> (2), so `a <=> b => c` is `(a <=> b) => c` and
    // `a => b <=> c` is `a => (b <=> c)`; neither chains with itself
    PNodeP expr() {
        PNodeP a = equiv();
        if (is("=>")) {
            const Tok op = v[i++];
            return bin(op, "=>", a, equiv());
        }
        return a;
    }
    PNodeP equiv() {
        PNodeP a = disj();
        if (is_any({"<=>", "\\equiv"})) {
            const Tok op = v[i++];
            return bin(op, "<=>", a, disj());
        }
        return a;
    }
    PNodeP disj() {
        PNodeP a = conj();
        while (is_any({"\\/", "\\lor"})) {
            const Tok op = v[i++];
            a = bin(op, "\\/", a, conj());
        }
        return a;
    }
    PNodeP conj() {
        PNodeP a = neg();
        while (is_any({"/\\", "\\land"})) {
            const Tok op = v[i++];
            a = bin(op, "/\\", a, neg());
        }
        return a;
    }
    PNodeP neg() {
        if (is_any({"~", "\\lnot", "\\neg"})) {
            const Tok op = v[i++];
            PNodeP n = node(PNode::NOT, op);
            n->k = {neg()};
            return n;
        }
        return cmp();
    }
    PNodeP cmp() {
        PNodeP a = setop();
        static const std::map<std::string, std::string> ops = {
            {"=", "="}, {"/=", "/="}, {"#", "/="}, {"<", "<"}, {"<=", "<="}, {"=<", "<="}, {"\\leq", "<="},
            {">", ">"}, {">=", ">="}, {"\\geq", ">="}, {"\\in", "\\in"}, {"\\notin", "\\notin"},
            {"\\subseteq", "\\subseteq"}};
        const Tok* p = peek();
        if (p) {
            auto it = ops.find(p->t);
            if (it != ops.end()) {
                const Tok op = v[i++];
                return bin(op, it->second, a, setop());
            }
        }
        return a;
    }
    PNodeP setop() {
        PNodeP a = range();
        for (;;) {
            const char* name = is_any({"\\cup", "\\union"}) ? "\\cup" : is_any({"\\cap", "\\intersect"}) ? "\\cap"
                               : is("\\") ? "\\" : nullptr;
            if (!name) return a;
            const Tok op = v[i++];
            a = bin(op, name, a, range());
        }
    }
    PNodeP range() {
        PNodeP a = add();
        if (is("..")) {
            const Tok op = v[i++];
            PNodeP n = node(PNode::RANGE, op);
            n->k = {a, add()};
            return n;
        }
        return a;
    }
    PNodeP add() {
        PNodeP a = postfix();
        while (is_any({"+", "-"})) {
            const Tok op = v[i++];
            a = bin(op, op.t, a, postfix());
        }
        return a;
    }
    PNodeP postfix() {
        PNodeP a = atom();
        for (;;) {
            if (is("[")) {
                const Tok op = v[i++];
                PNodeP n = node(PNode::INDEX, op);
                n->k = {a, expr()};
                expect("]");
                a = n;
            } else if (is(".")) {
                const Tok op = v[i++];
                const Tok* f = peek();
                if (!f || !ident_tok(f->t)) refuse("expected a field name after `.`", f);
                PNodeP n = node(PNode::FIELD, op, f->t);
                ++i;
                n->k = {a};
                a = n;
            } else if (is("'")) {
                if (!primes) refuse("a primed variable (a state predicate reads one state)", peek());
                const Tok op = v[i++];
                PNodeP n = node(PNode::PRIME, op);
                n->k = {a};
                a = n;
            } else {
                return a;
            }
        }
    }
    PNodeP junction(const std::string& bullet) {
        const int col = peek()->col;
        const Tok first = *peek();
        PNodeP acc;
        while (peek() && (peek()->t == bullet) && peek()->col == col) {
            ++i;
            margin.push_back(col);
            PNodeP item = expr();
            margin.pop_back();
            acc = acc ? bin(first, bullet, acc, item) : item;
        }
        return acc;
    }
    PNodeP atom() {
        const Tok* p = peek();
        if (!p) refuse("an expression is missing", nullptr);
        const Tok t = *p;
        if (t.t == "/\\" || t.t == "\\/") return junction(t.t);
        if (t.t == "\\land" || t.t == "\\lor") refuse("a junction list bulleted with " + t.t + " (write /\\ or \\/)", p);
        if (isdigit((unsigned char)t.t[0])) {
            ++i;
            return node(PNode::NUM, t, t.t);
        }
        if (t.t == "-" && i + 1 < v.size() && isdigit((unsigned char)v[i + 1].t[0])) {
            i += 2;
            return node(PNode::NUM, t, "-" + v[i - 1].t);
        }
        if (t.t == "(") {
            ++i;
            PNodeP n = expr();
            expect(")");
            return n;
        }
        if (t.t == "{") return braces();
        if (t.t == "IF") {
            ++i;
            PNodeP n = node(PNode::IF, t);
            PNodeP c = expr();
            expect("THEN");
            PNodeP a = expr();
            expect("ELSE");
            PNodeP b = expr();
            n->k = {c, a, b};
            return n;
        }
        if (t.t == "\\A" || t.t == "\\E") return quant();
        if (t.t == "DOMAIN") {
            ++i;
            PNodeP n = node(PNode::DOMAIN, t);
            n->k = {postfix()};
            return n;
        }
        for (const char* kw : {"LET", "CHOOSE", "CASE", "EXCEPT", "LAMBDA", "ENABLED", "UNCHANGED", "SUBSET", "UNION",
                               "\\AA", "\\EE"})
            if (t.t == kw) refuse(t.t, p);
        if (t.t[0] == '"') refuse("a string " + t.t, p);
        if (t.t == "<<") refuse("a tuple or sequence <<...>>", p);
        if (t.t == "[") {
            for (size_t q = i; q < v.size() && v[q].t != "]"; ++q)
                if (v[q].t == "EXCEPT") refuse("EXCEPT", &v[q]);
            refuse("a function or record constructor [...]", p);
        }
        if (ident_tok(t.t)) {
            ++i;
            if (is("(")) {
                ++i;
                PNodeP n = node(PNode::CALL, t, t.t);
                if (!is(")"))
                    for (;;) {
                        n->k.push_back(expr());
                        if (is(",")) { ++i; continue; }
                        break;
                    }
                expect(")");
                return n;
            }
            return node(PNode::ID, t, t.t);
        }
        refuse("unexpected `" + t.t + "`", p);
    }
    PNodeP braces() {
        const Tok open = expect("{");
        if (is("}")) {
            ++i;
            return node(PNode::SETLIT, open);
        }
        // {x \in D : P}
        if (peek() && ident_tok(peek()->t) && i + 1 < v.size() && v[i + 1].t == "\\in") {
            const size_t save = i;
            const Tok name = v[i];
            i += 2;
            PNodeP dom = setop();
            if (is(":")) {
                ++i;
                PNodeP n = node(PNode::SETCOMP, open, name.t);
                PNodeP body = expr();
                n->k = {dom, body};
                expect("}");
                return n;
            }
            i = save;
        }
        PNodeP n = node(PNode::SETLIT, open);
        for (;;) {
            n->k.push_back(expr());
            if (is(",")) { ++i; continue; }
            break;
        }
        if (is(":")) refuse("a set constructor {e : x \\in S}", peek());
        expect("}");
        return n;
    }
    PNodeP quant() {
        const Tok q = v[i++];
        PNodeP n = node(PNode::QUANT, q, q.t);
        for (;;) {  // groups `a, b \in D`
            std::vector<std::string> group;
            for (;;) {
                const Tok* p = peek();
                if (!p || !ident_tok(p->t)) refuse("expected a bound name", p);
                group.push_back(p->t);
                ++i;
                if (is(",")) { ++i; continue; }
                break;
            }
            if (!is("\\in")) refuse("an unbounded quantifier (" + q.t + " " + group[0] + " without \\in)", peek());
            ++i;
            PNodeP dom = setop();
            for (const auto& g : group) {
                n->names.push_back(g);
                n->k.push_back(dom);
            }
            if (is(",")) { ++i; continue; }
            break;
        }
        expect(":");
        n->k.push_back(expr());
        return n;
    }
};

// ---- generator ----------------------------------------------------------------------------
enum PTy { T_BOOL, T_INT, T_SERVER, T_NIL, T_ROLE, T_MTYPE, T_SET, T_MSG, T_VALUE };
inline const char* ty_name(PTy t) {
    static const char* n[] = {"Boolean", "integer", "server", "Nil", "role", "message type", "set of servers",
                              "message", "Value"};
    return n[t];
}

struct PEnv;
struct PBinding {
    int reg = -1;   // a bound name's register, or -1: a definition's parameter
    PTy ty = T_INT;
    bool bagp = false;  // a bound message: a slot of the successor's bag (\A m \in DOMAIN messages')
    PNodeP arg;     // parameter: the argument, generated in the caller's scope
    const PEnv* env = nullptr;
};
struct PEnv {
    std::map<std::string, PBinding> m;
    const PEnv* parent = nullptr;
    const PBinding* find(const std::string& n) const {
        for (const PEnv* e = this; e; e = e->parent) {
            auto it = e->m.find(n);
            if (it != e->m.end()) return &it->second;
        }
        return nullptr;
    }
};

class PredGen {
    const Ctx& X;
    const std::vector<std::string>& servers;
    const std::vector<std::string>& values;
    std::vector<uint32_t>& code;
    int depth = 0, max_depth = 0, nreg = 0, max_reg = 0;
    std::vector<std::string> expanding;
    using Op = rmc::pred::Op;
    bool actions = false;  // an action property's body: primes are in the language
    bool msg_bagp = false;  // the bag of the bound message loaded last (gen_id)
    bool primed = false;   // inside a primed expression: every state read is of the successor
    // a state read of the state the expression is in (or of the successor: a primed variable)
    static Op rd(Op op, bool next) { return (Op)((uint32_t)op | (next ? rmc::pred::OP_PRIMED : 0u)); }
    struct PrimeScope {  // primes what is generated while it lives
        PredGen& g;
        bool was;
        PrimeScope(PredGen& gen, bool on) : g(gen), was(gen.primed) { g.primed = was || on; }
        ~PrimeScope() { g.primed = was; }
    };

public:
    int names_server = 0;

    PredGen(const Ctx& x, const std::vector<std::string>& sv, const std::vector<std::string>& vv,
            std::vector<uint32_t>& out)
        : X(x), servers(sv), values(vv), code(out) {}
    int stack_depth() const { return max_depth; }
    int bound_names() const { return max_reg; }
    void set_actions(bool on) { actions = on; }

    void predicate(const std::string& name) {
        PEnv top;
        depth = 0;
        const PTy t = expand(name, {}, nullptr, top, 0, 0);
        if (t != T_BOOL) throw PredError{"the predicate is not Boolean (it is a " + std::string(ty_name(t)) + ")"};
        emit(rmc::pred::OP_HALT, 0, 0);
    }
    // a CONSTRAINT's residual conjunct: its tokens as they stand in the model (no parameters in scope)
    void residual(const std::vector<Tok>& toks) {
        PEnv top;
        depth = 0;
        primed = false;
        const PTy t = gen(PredParser(toks, actions).parse_all(), top);
        if (t != T_BOOL) throw PredError{"the conjunct is not Boolean (it is a " + std::string(ty_name(t)) + ")"};
        emit(rmc::pred::OP_HALT, 0, 0);
    }

private:
    [[noreturn]] static void refuse(const std::string& what, const PNodeP& n) {
        throw PredError{what + at_of(n->line, n->col)};
    }
    size_t emit(Op op, int arg, int delta) {
        code.push_back(rmc::pred::ins(op, arg));
        depth += delta;
        max_depth = std::max(max_depth, depth);
        return code.size() - 1;
    }
    void patch(size_t at, int target) { code[at] = (code[at] & 255u) | ((uint32_t)target << 8); }
    void patch_loop(size_t at, int target, int reg) { patch(at, (target << 3) | reg); }
    int here() const { return (int)code.size(); }
    int new_reg() {
        const int r = nreg++;
        max_reg = std::max(max_reg, nreg);
        return r;
    }
    void want(PTy got, PTy need, const PNodeP& n, const char* where) {
        if (got == need || (need == T_SERVER && got == T_NIL)) return;
        refuse(std::string(where) + " must be a " + ty_name(need) + ", not a " + ty_name(got), n);
    }

    // a reference to a model definition: its body, parsed, with the parameters bound
    PTy expand(const std::string& name, const std::vector<PNodeP>& args, const PNodeP& site, const PEnv& env, int line,
               int col) {
        const Unit* u = X.def(name);
        auto where = [&] { return site ? at_of(site->line, site->col) : std::string(); };
        if (!u) throw PredError{"unknown identifier " + name + where()};
        for (const auto& e : expanding)
            if (e == name) throw PredError{"recursive definition " + name + where()};
        if (expanding.size() > 32) throw PredError{"definitions nest too deeply at " + name + where()};
        std::vector<std::string> params;
        {
            std::smatch m;
            std::string head = u->lines.empty() ? "" : u->lines[0].second;
            if (std::regex_search(head, m, kDefRe) && m[3].matched) {
                std::string p = m[3].str();
                p = p.substr(1, p.size() - 2);
                std::stringstream ss(p);
                std::string tok;
                while (std::getline(ss, tok, ',')) params.push_back(trim(tok));
            }
        }
        if (params.size() != args.size())
            throw PredError{name + " takes " + std::to_string(params.size()) + " argument(s), given " +
                            std::to_string(args.size()) + where()};
        for (const auto& p : params)
            if (p.find('(') != std::string::npos || p.find('_') != std::string::npos)
                throw PredError{"an operator parameter of " + name + where()};
        const std::vector<Tok> toks = tokenize(*u, true);
        PNodeP body;
        try {
            body = PredParser(toks, actions).parse_all();
        } catch (PredError& e) {
            e.msg = "in " + name + ": " + e.msg;
            throw;
        }
        PEnv inner;  // a definition is closed: it sees its parameters only
        for (size_t q = 0; q < params.size(); ++q) {
            PBinding b;
            b.arg = args[q];
            b.env = &env;
            inner.m[params[q]] = b;
        }
        expanding.push_back(name);
        PTy t;
        try {
            t = gen(body, inner);
        } catch (PredError& e) {
            if (e.msg.rfind("in ", 0) != 0 && site) e.msg = "in " + name + ": " + e.msg;
            throw;
        }
        expanding.pop_back();
        (void)line;
        (void)col;
        return t;
    }

    static bool is_id(const PNodeP& n, const char* s) { return n->kind == PNode::ID && n->s == s; }
    // log[i]: the server expression, or null
    // (*pr: the variable is primed, log'[i])
    PNodeP log_of(const PNodeP& n, bool* pr) const {
        if (n->kind != PNode::INDEX) return nullptr;
        const PNodeP v = var_of(n->k[0], pr);
        return is_id(v, "log") ? n->k[1] : nullptr;
    }
    // a variable as written, x or x': the ID, and whether it is primed (a prime inside a primed
    // expression is refused)
    PNodeP var_of(const PNodeP& n, bool* pr) const {
        *pr = false;
        if (n->kind != PNode::PRIME || n->k[0]->kind != PNode::ID) return n;
        if (primed) refuse("a prime inside an already primed expression", n);
        *pr = true;
        return n->k[0];
    }
    // through a parameter to the argument it stands for (so Len(l) with l <- log[i] reads as written out)
    PNodeP resolve(PNodeP n, const PEnv*& env) const {
        while (n->kind == PNode::ID) {
            const PBinding* b = env->find(n->s);
            if (!b || b->reg >= 0) break;
            n = b->arg;
            env = b->env;
        }
        return n;
    }

    void gen_server(const PNodeP& n, const PEnv& env, const char* where) { want(gen(n, env), T_SERVER, n, where); }

    struct Domain {
        Op iter, next;
        PTy ty;
        bool bagp = false;  // T_MSG: the slots are of the successor's bag
    };
    // the code that sets up a quantifier's domain (left on the stack for the ITER instruction)
    Domain gen_domain(const PNodeP& d0, const PEnv& env0) {
        const PEnv* envp = &env0;
        const PNodeP d = resolve(d0, envp);
        const PEnv& env = *envp;
        using namespace rmc::pred;
        if (is_id(d, "Quorum")) return {OP_ITER_QUORUM, OP_NEXT_QUORUM, T_SET};
        if (d->kind == PNode::RANGE) {
            want(gen(d->k[0], env), T_INT, d->k[0], "the lower end of a range");
            want(gen(d->k[1], env), T_INT, d->k[1], "the upper end of a range");
            return {OP_ITER_RANGE, OP_NEXT_RANGE, T_INT};
        }
        if (d->kind == PNode::BIN && d->s == "\\cap" && d->k[0]->kind == PNode::RANGE && d->k[1]->kind == PNode::RANGE) {
            want(gen(d->k[0]->k[0], env), T_INT, d->k[0], "the lower end of a range");
            want(gen(d->k[1]->k[0], env), T_INT, d->k[1], "the lower end of a range");
            emit(OP_MAX, 0, -1);
            want(gen(d->k[0]->k[1], env), T_INT, d->k[0], "the upper end of a range");
            want(gen(d->k[1]->k[1], env), T_INT, d->k[1], "the upper end of a range");
            emit(OP_MIN, 0, -1);
            return {OP_ITER_RANGE, OP_NEXT_RANGE, T_INT};
        }
        if (d->kind == PNode::DOMAIN) {
            const PEnv* e2 = &env;
            const PNodeP x = resolve(d->k[0], e2);
            bool pr = false;
            if (is_id(var_of(x, &pr), "messages")) {
                emit(OP_PUSH, 0, 1);
                emit(rd(OP_NMSG, primed || pr), 0, 1);
                emit(OP_PUSH, 1, 1);
                emit(OP_SUB, 0, -1);
                return {OP_ITER_RANGE, OP_NEXT_RANGE, T_MSG, primed || pr};
            }
            if (PNodeP i = log_of(x, &pr)) {
                emit(OP_PUSH, 1, 1);
                gen_server(i, *e2, "the index of log");
                emit(rd(OP_LEN, primed || pr), 0, 0);
                return {OP_ITER_RANGE, OP_NEXT_RANGE, T_INT};
            }
            refuse("DOMAIN of anything but messages or log[i]", d);
        }
        want(gen(d, env), T_SET, d, "a quantifier's domain");
        return {OP_ITER_SET, OP_NEXT_SET, T_SERVER};
    }

    PTy gen_quant(const PNodeP& n, const PEnv& env, size_t k) {
        using namespace rmc::pred;
        if (k == n->names.size()) {
            const PTy t = gen(n->k.back(), env);
            want(t, T_BOOL, n->k.back(), "a quantifier's body");
            return T_BOOL;
        }
        const bool all = n->s == "\\A";
        const Domain dm = gen_domain(n->k[k], env);
        const int r = new_reg();
        if (r >= PRED_BOUND) refuse(std::to_string(r + 1) + " bound names in scope exceed 8:", n);
        emit(dm.iter, r, dm.iter == OP_ITER_QUORUM ? 0 : dm.iter == OP_ITER_SET ? -1 : -2);
        const int d0 = depth;
        const int loop = here();
        const size_t nx = emit(dm.next, 0, 0);
        PEnv inner;
        inner.parent = &env;
        PBinding b;
        b.reg = r;
        b.ty = dm.ty;
        b.bagp = dm.bagp;
        inner.m[n->names[k]] = b;
        gen_quant(n, inner, k + 1);
        emit(all ? OP_JT : OP_JF, loop, -1);  // \A: a true body goes on; \E: a false one
        emit(OP_PUSH, all ? 0 : 1, 1);
        const size_t out = emit(OP_JMP, 0, 0);
        depth = d0;
        patch_loop(nx, here(), r);
        emit(OP_PUSH, all ? 1 : 0, 1);
        patch(out, here());
        --nreg;
        return T_BOOL;
    }

    PTy gen_in(const PNodeP& n, const PEnv& env) {
        using namespace rmc::pred;
        const PEnv* envp = &env;
        const PNodeP r = resolve(n->k[1], envp);
        if (is_id(r, "Quorum")) {
            want(gen(n->k[0], env), T_SET, n->k[0], "the left of \\in Quorum");
            emit(OP_ISQUORUM, 0, 0);
            return T_BOOL;
        }
        if (r->kind == PNode::RANGE) {
            want(gen(n->k[0], env), T_INT, n->k[0], "the left of \\in a..b");
            want(gen(r->k[0], *envp), T_INT, r->k[0], "the lower end of a range");
            want(gen(r->k[1], *envp), T_INT, r->k[1], "the upper end of a range");
            emit(OP_INRANGE, 0, -2);
            return T_BOOL;
        }
        if (r->kind == PNode::DOMAIN) {
            const PEnv* e2 = envp;
            const PNodeP x = resolve(r->k[0], e2);
            bool pr = false;
            if (PNodeP i = log_of(x, &pr)) {
                want(gen(n->k[0], env), T_INT, n->k[0], "the left of \\in DOMAIN log[i]");
                emit(OP_PUSH, 1, 1);
                gen_server(i, *e2, "the index of log");
                emit(rd(OP_LEN, primed || pr), 0, 0);
                emit(OP_INRANGE, 0, -2);
                return T_BOOL;
            }
            refuse("\\in DOMAIN of anything but log[i]", r);
        }
        const PTy lt = gen(n->k[0], env);
        if (lt != T_SERVER && lt != T_NIL) refuse(std::string("the left of \\in must be a server, not a ") + ty_name(lt), n->k[0]);
        want(gen(r, *envp), T_SET, n->k[1], "the right of \\in");
        emit(OP_IN, 0, -1);
        return T_BOOL;
    }

    PTy gen_bin(const PNodeP& n, const PEnv& env) {
        using namespace rmc::pred;
        const std::string& op = n->s;
        if (op == "/\\" || op == "\\/" || op == "=>") {
            want(gen(n->k[0], env), T_BOOL, n->k[0], ("the left of " + op).c_str());
            if (op == "=>") emit(OP_NOT, 0, 0);
            const size_t j = emit(op == "/\\" ? OP_AND_SC : OP_OR_SC, 0, -1);
            want(gen(n->k[1], env), T_BOOL, n->k[1], ("the right of " + op).c_str());
            patch(j, here());
            return T_BOOL;
        }
        if (op == "<=>") {
            want(gen(n->k[0], env), T_BOOL, n->k[0], "the left of <=>");
            want(gen(n->k[1], env), T_BOOL, n->k[1], "the right of <=>");
            emit(OP_EQ, 0, -1);
            return T_BOOL;
        }
        if (op == "\\in" || op == "\\notin") {
            gen_in(n, env);
            if (op == "\\notin") emit(OP_NOT, 0, 0);
            return T_BOOL;
        }
        if (op == "=" || op == "/=") {
            const PTy a = gen(n->k[0], env), b = gen(n->k[1], env);
            const bool srv = (a == T_SERVER || a == T_NIL) && (b == T_SERVER || b == T_NIL);
            if (a == T_MSG || b == T_MSG) refuse("record equality (compare a message's fields)", n);
            if (!srv && a != b)
                refuse(std::string("`") + op + "` between a " + ty_name(a) + " and a " + ty_name(b), n);
            emit(op == "=" ? OP_EQ : OP_NE, 0, -1);
            return T_BOOL;
        }
        if (op == "<" || op == "<=" || op == ">" || op == ">=") {
            want(gen(n->k[0], env), T_INT, n->k[0], ("the left of " + op).c_str());
            want(gen(n->k[1], env), T_INT, n->k[1], ("the right of " + op).c_str());
            emit(op == "<" ? OP_LT : op == "<=" ? OP_LE : op == ">" ? OP_GT : OP_GE, 0, -1);
            return T_BOOL;
        }
        if (op == "+" || op == "-") {
            want(gen(n->k[0], env), T_INT, n->k[0], ("the left of " + op).c_str());
            want(gen(n->k[1], env), T_INT, n->k[1], ("the right of " + op).c_str());
            emit(op == "+" ? OP_ADD : OP_SUB, 0, -1);
            return T_INT;
        }
        if (op == "\\cup" || op == "\\cap" || op == "\\" || op == "\\subseteq") {
            want(gen(n->k[0], env), T_SET, n->k[0], ("the left of " + op).c_str());
            want(gen(n->k[1], env), T_SET, n->k[1], ("the right of " + op).c_str());
            emit(op == "\\cup" ? OP_OR : op == "\\cap" ? OP_AND : op == "\\" ? OP_ANDN : OP_SUBSET, 0, -1);
            return op == "\\subseteq" ? T_BOOL : T_SET;
        }
        refuse("operator " + op, n);
    }

    PTy gen_id(const PNodeP& n, const PEnv& env) {
        using namespace rmc::pred;
        const std::string& s = n->s;
        if (const PBinding* b = env.find(s)) {
            if (b->reg >= 0) {
                emit(OP_LOAD, b->reg, 1);
                msg_bagp = b->bagp;
                return b->ty;
            }
            return gen(b->arg, *b->env);
        }
        static const std::map<std::string, std::pair<int, PTy>> atoms = {
            {"TRUE", {1, T_BOOL}}, {"FALSE", {0, T_BOOL}}, {"Nil", {-1, T_NIL}},
            {"Follower", {0, T_ROLE}}, {"Candidate", {1, T_ROLE}}, {"Leader", {2, T_ROLE}},
            {"RequestVoteRequest", {0, T_MTYPE}}, {"RequestVoteResponse", {1, T_MTYPE}},
            {"AppendEntriesRequest", {2, T_MTYPE}}, {"AppendEntriesResponse", {3, T_MTYPE}}};
        auto it = atoms.find(s);
        if (it != atoms.end()) {
            emit(OP_PUSH, it->second.first, 1);
            return it->second.second;
        }
        if (s == "Server") {
            emit(OP_PUSH, (1 << (int)servers.size()) - 1, 1);
            return T_SET;
        }
        if (s == "Quorum") refuse("Quorum (accepted to the right of \\in and as a quantifier's domain)", n);
        for (size_t q = 0; q < servers.size(); ++q)
            if (servers[q] == s) {
                names_server = 1;
                emit(OP_PUSH, (int)q, 1);
                return T_SERVER;
            }
        for (const auto& vname : values)
            if (vname == s) refuse("a Value-typed comparison (model value " + s + ")", n);
        if (s == "Value") refuse("a Value-typed comparison (Value)", n);
        for (const char* sv : kStateVars)
            if (s == sv)
                refuse("the variable " + s + " as a whole (function, sequence or record equality is not in the language; "
                       "read " + s + "[...])", n);
        int val = 0;
        if (X.int_of(s, &val)) {
            if (val < -(1 << 22) || val >= (1 << 22)) refuse("an integer beyond 22 bits", n);
            emit(OP_PUSH, val, 1);
            return T_INT;
        }
        if (X.def(s)) return expand(s, {}, n, env, n->line, n->col);
        for (const auto& u : kRaftUnits)
            if (u.name[0] && s == u.name) refuse("raft.tla's " + s, n);
        refuse("unknown identifier " + s, n);
    }

    PTy gen(const PNodeP& n, const PEnv& env) {
        using namespace rmc::pred;
        switch (n->kind) {
            case PNode::NUM: {
                const long x = strtol(n->s.c_str(), nullptr, 10);
                if (x < -(1 << 22) || x >= (1 << 22)) refuse("an integer beyond 22 bits", n);
                emit(OP_PUSH, (int)x, 1);
                return T_INT;
            }
            case PNode::ID: return gen_id(n, env);
            case PNode::NOT:
                want(gen(n->k[0], env), T_BOOL, n->k[0], "the operand of ~");
                emit(OP_NOT, 0, 0);
                return T_BOOL;
            case PNode::BIN: return gen_bin(n, env);
            case PNode::IF: {
                want(gen(n->k[0], env), T_BOOL, n->k[0], "the condition of IF");
                const size_t jf = emit(OP_JF, 0, -1);
                const int d0 = depth;
                const PTy a = gen(n->k[1], env);
                const size_t out = emit(OP_JMP, 0, 0);
                depth = d0;
                patch(jf, here());
                const PTy b = gen(n->k[2], env);
                patch(out, here());
                const bool srv = (a == T_SERVER || a == T_NIL) && (b == T_SERVER || b == T_NIL);
                if (!srv && a != b)
                    refuse(std::string("IF whose branches are a ") + ty_name(a) + " and a " + ty_name(b), n);
                return srv ? T_SERVER : a;
            }
            case PNode::QUANT: return gen_quant(n, env, 0);
            case PNode::SETLIT:
                emit(OP_PUSH, 0, 1);
                for (const auto& e : n->k) {
                    const PTy t = gen(e, env);
                    if (t != T_SERVER && t != T_NIL)
                        refuse(std::string("a set literal's element must be a server or Nil, not a ") + ty_name(t), e);
                    emit(OP_BIT, 0, 0);
                    emit(OP_OR, 0, -1);
                }
                return T_SET;
            case PNode::SETCOMP: {
                emit(OP_PUSH, 0, 1);
                const Domain dm = gen_domain(n->k[0], env);
                if (dm.iter != OP_ITER_SET) refuse("{x \\in D : P} over anything but a set of servers", n);
                const int r = new_reg();
                if (r >= PRED_BOUND) refuse(std::to_string(r + 1) + " bound names in scope exceed 8:", n);
                emit(OP_ITER_SET, r, -1);
                const int loop = here();
                const size_t nx = emit(OP_NEXT_SET, 0, 0);
                PEnv inner;
                inner.parent = &env;
                PBinding b;
                b.reg = r;
                b.ty = T_SERVER;
                inner.m[n->s] = b;
                want(gen(n->k[1], inner), T_BOOL, n->k[1], "the condition of {x \\in D : P}");
                emit(OP_JF, loop, -1);
                emit(OP_LOAD, r, 1);
                emit(OP_BIT, 0, 0);
                emit(OP_OR, 0, -1);
                emit(OP_JMP, loop, 0);
                patch_loop(nx, here(), r);
                --nreg;
                return T_SET;
            }
            case PNode::RANGE: refuse("a..b (accepted to the right of \\in and as a quantifier's domain)", n);
            case PNode::DOMAIN: refuse("DOMAIN (accepted to the right of \\in and as a quantifier's domain)", n);
            case PNode::INDEX: return gen_index(n, env);
            case PNode::FIELD: return gen_field(n, env);
            case PNode::CALL: return gen_call(n, env);
            case PNode::PRIME: {
                if (primed) refuse("a prime inside an already primed expression", n);
                PrimeScope ps(*this, true);
                return gen(n->k[0], env);
            }
        }
        refuse("this construct", n);
    }

    PTy gen_index(const PNodeP& n, const PEnv& env0) {
        using namespace rmc::pred;
        const PEnv* envp = &env0;
        bool pr = false;
        const PNodeP base = var_of(resolve(n->k[0], envp), &pr);
        const bool nx = primed || pr;
        static const std::map<std::string, std::pair<Op, PTy>> vars = {
            {"currentTerm", {OP_TERM, T_INT}}, {"state", {OP_ROLE, T_ROLE}}, {"votedFor", {OP_VOTED, T_SERVER}},
            {"commitIndex", {OP_COMMIT, T_INT}}, {"votesResponded", {OP_VRESP, T_SET}},
            {"votesGranted", {OP_VGRANT, T_SET}}};
        if (base->kind == PNode::ID && !envp->find(base->s)) {
            auto it = vars.find(base->s);
            if (it != vars.end()) {
                gen_server(n->k[1], env0, ("the index of " + base->s).c_str());
                emit(rd(it->second.first, nx), 0, 0);
                return it->second.second;
            }
            if (base->s == "messages") {
                want(gen(n->k[1], env0), T_MSG, n->k[1], "the index of messages");
                if (msg_bagp != nx)
                    refuse(std::string("a message bound in ") + (msg_bagp ? "DOMAIN messages'" : "DOMAIN messages") +
                           " as an index of " + (nx ? "messages'" : "messages") + " (a bound message is a slot of the bag "
                           "it was bound in)", n);
                emit(rd(OP_MSGCNT, nx), 0, 0);
                return T_INT;
            }
            if (base->s == "log")
                refuse("the sequence log[i] as a value (read Len(log[i]), LastTerm(log[i]), DOMAIN log[i], "
                       "log[i][n].term or log[i][n].value; sequence equality is not in the language)", n);
            if (base->s == "nextIndex" || base->s == "matchIndex")
                refuse("the function " + base->s + "[i] as a value (read " + base->s + "[i][j])", n);
        }
        if (base->kind == PNode::INDEX) {
            const PEnv* e2 = envp;
            bool pr2 = false;
            const PNodeP bb = var_of(resolve(base->k[0], e2), &pr2);
            if (is_id(bb, "nextIndex") || is_id(bb, "matchIndex")) {
                gen_server(base->k[1], *envp, "the first index");
                gen_server(n->k[1], env0, "the second index");
                emit(rd(is_id(bb, "nextIndex") ? OP_NEXT : OP_MATCH, primed || pr2), 0, -1);
                return T_INT;
            }
            if (is_id(bb, "log"))
                refuse("the record log[i][n] as a value (read its .term or .value; record equality is not in the language)", n);
        }
        refuse("function application of anything but a variable of raft.tla", n);
    }

    PTy gen_field(const PNodeP& n, const PEnv& env0) {
        using namespace rmc::pred;
        const PEnv* envp = &env0;
        const PNodeP base = resolve(n->k[0], envp);
        if (base->kind == PNode::INDEX) {  // log[i][n].term / .value
            const PEnv* e2 = envp;
            const PNodeP inner = resolve(base->k[0], e2);
            bool pr = false;
            if (PNodeP i = log_of(inner, &pr)) {
                if (n->s != "term" && n->s != "value") refuse("field ." + n->s + " of a log entry (term, value)", n);
                gen_server(i, *e2, "the index of log");
                want(gen(base->k[1], *envp), T_INT, base->k[1], "the position in log[i]");
                emit(rd(n->s == "term" ? OP_LOGTERM : OP_LOGVAL, primed || pr), 0, -1);
                return n->s == "term" ? T_INT : T_VALUE;
            }
        }
        static const std::map<std::string, std::pair<int, PTy>> fields = {
            {"mtype", {F_MTYPE, T_MTYPE}}, {"mterm", {F_MTERM, T_INT}}, {"msource", {F_MSOURCE, T_SERVER}},
            {"mdest", {F_MDEST, T_SERVER}}, {"mlastLogTerm", {F_MLASTLOGTERM, T_INT}},
            {"mlastLogIndex", {F_MLASTLOGINDEX, T_INT}}, {"mvoteGranted", {F_MVOTEGRANTED, T_BOOL}},
            {"mprevLogIndex", {F_MPREVLOGINDEX, T_INT}}, {"mprevLogTerm", {F_MPREVLOGTERM, T_INT}},
            {"mcommitIndex", {F_MCOMMITINDEX, T_INT}}, {"msuccess", {F_MSUCCESS, T_BOOL}},
            {"mmatchIndex", {F_MMATCHINDEX, T_INT}}};
        if (n->s == "mentries" || n->s == "mlog") refuse("m." + n->s + " (a sequence-valued message field)", n);
        auto it = fields.find(n->s);
        if (it == fields.end()) refuse("field ." + n->s, n);
        const PTy t = gen(n->k[0], env0);
        if (t != T_MSG) refuse(std::string("field .") + n->s + " of a " + ty_name(t), n);
        emit(rd(OP_MSGF, msg_bagp), it->second.first, 0);  // (the bag it was bound in, primed or not here)
        return it->second.second;
    }

    PTy gen_call(const PNodeP& n, const PEnv& env) {
        using namespace rmc::pred;
        const std::string& f = n->s;
        if (f == "Len" || f == "LastTerm") {
            if (n->k.size() != 1) refuse(f + " takes one argument", n);
            const PEnv* e2 = &env;
            const PNodeP x = resolve(n->k[0], e2);
            bool pr = false;
            PNodeP i = log_of(x, &pr);
            if (!i) refuse(f + " of anything but log[i]", n);
            gen_server(i, *e2, "the index of log");
            emit(rd(f == "Len" ? OP_LEN : OP_LASTTERM, primed || pr), 0, 0);
            return T_INT;
        }
        if (f == "Cardinality") {
            if (n->k.size() != 1) refuse("Cardinality takes one argument", n);
            const PEnv* e2 = &env;
            const PNodeP x = resolve(n->k[0], e2);
            if (x->kind == PNode::DOMAIN) {
                const PEnv* e3 = e2;
                bool pr = false;
                if (is_id(var_of(resolve(x->k[0], e3), &pr), "messages")) {
                    emit(rd(OP_NMSG, primed || pr), 0, 1);
                    return T_INT;
                }
            }
            want(gen(n->k[0], env), T_SET, n->k[0], "the argument of Cardinality");
            emit(OP_CARD, 0, 0);
            return T_INT;
        }
        for (const char* lib : {"SubSeq", "Append", "Head", "Tail", "Seq", "BagToSet", "SetToBag", "Permutations",
                                "IsPrefix", "Min", "Max", "WithMessage", "WithoutMessage"})
            if (f == lib) refuse(f, n);
        if (X.def(f)) return expand(f, n->k, n, env, n->line, n->col);
        for (const auto& u : kRaftUnits)
            if (u.name[0] && f == u.name) refuse("raft.tla's " + f, n);
        refuse("unknown identifier " + f, n);
    }
};

// One predicate of a program: an INVARIANT (a definition of the model, toks == nullptr) or a
// CONSTRAINT's residual conjunct (its tokens).
struct PredItem {
    std::string name, label;  // the program's name of it; how messages call it
    const std::vector<Tok>* toks;
};

// A conjunct of a CONSTRAINT that is no bound (rmc_front.cpp, RMC_FRONT_CONSTRAINTS).
struct Residual {
    std::string name;  // the cfg's CONSTRAINT it came from
    std::vector<Tok> toks;
    std::string text;
    int line = 0;
};

// Compiles `items` into *out; on failure the message names the item, the construct, and its
// line and column.  what: "model-defined invariants" / "residual constraint conjuncts".
inline bool compile_program(const Ctx& X, const std::vector<PredItem>& items, const char* what,
                            const std::vector<std::string>& servers, const std::vector<std::string>& values,
                            rmc_predicates* out, std::string* err, bool actions = false) {
    using namespace rmc::pred;
    memset(out, 0, sizeof *out);
    out->prog.n_servers = (int)servers.size();
    out->actions = actions ? 1 : 0;
    if (actions && (int)items.size() > RMC_MAX_ACTION_PROPS) {
        *err = std::to_string(items.size()) + " " + what + " exceed RMC_MAX_ACTION_PROPS = " +
               std::to_string(RMC_MAX_ACTION_PROPS);
        return false;
    }
    if ((int)items.size() > PRED_MAX) {
        *err = std::to_string(items.size()) + " " + what + " exceed RMC_MAX_PREDICATES = " + std::to_string(PRED_MAX);
        return false;
    }
    std::vector<uint32_t> code;
    PredGen g(X, servers, values, code);
    g.set_actions(actions);
    for (size_t p = 0; p < items.size(); ++p) {
        const std::string& label = items[p].label;
        out->prog.entry[p] = (int)code.size();
        try {
            if (items[p].toks) g.residual(*items[p].toks);
            else g.predicate(items[p].name);
        } catch (const PredError& e) {
            *err = label + ": " + e.msg + " is not in the predicate language (rmc.h \"model-defined invariants\")";
            return false;
        }
        if (g.stack_depth() > PRED_STACK) {
            *err = label + ": evaluation stack depth " + std::to_string(g.stack_depth()) + " exceeds " +
                   std::to_string(PRED_STACK);
            return false;
        }
        if (g.bound_names() > PRED_BOUND) {
            *err = label + ": " + std::to_string(g.bound_names()) + " bound names exceed " + std::to_string(PRED_BOUND);
            return false;
        }
        if ((int)code.size() > PRED_CODE) {
            *err = label + ": " + std::to_string(code.size()) + " code words in all exceed " + std::to_string(PRED_CODE);
            return false;
        }
        snprintf(out->name[p], sizeof out->name[p], "%s", items[p].name.c_str());
    }
    out->prog.n_pred = (int)items.size();
    out->prog.n_code = (int)code.size();
    for (size_t q = 0; q < code.size(); ++q) out->prog.code[q] = code[q];
    out->names_server = g.names_server;
    return true;
}

// The INVARIANTs `names` (definitions of the model).
inline bool compile_predicates(const Ctx& X, const std::vector<std::string>& names,
                               const std::vector<std::string>& servers, const std::vector<std::string>& values,
                               rmc_predicates* out, std::string* err) {
    std::vector<PredItem> items;
    for (const auto& n : names) items.push_back({n, "INVARIANT " + n, nullptr});
    return compile_program(X, items, "model-defined invariants", servers, values, out, err);
}

// An action property of the cfg (PROPERTY P with P == [][A]_vars): its name and A's tokens.
struct ActionProp {
    std::string name;
    std::vector<Tok> toks;
};

// The model's action properties, in cfg order: each A with primes in the language.
inline bool compile_actions(const Ctx& X, const std::vector<ActionProp>& props, const std::vector<std::string>& servers,
                            const std::vector<std::string>& values, rmc_predicates* out, std::string* err) {
    std::vector<PredItem> items;
    for (const auto& a : props) items.push_back({a.name, "PROPERTY " + a.name, &a.toks});
    return compile_program(X, items, "action properties", servers, values, out, err, true);
}

// The residual conjuncts of the model's CONSTRAINTs, in order.
inline bool compile_residuals(const Ctx& X, const std::vector<Residual>& residuals,
                              const std::vector<std::string>& servers, const std::vector<std::string>& values,
                              rmc_predicates* out, std::string* err) {
    std::vector<PredItem> items;
    for (const auto& r : residuals)
        items.push_back({r.name, "CONSTRAINT " + r.name + ": conjunct `" + r.text + "`", &r.toks});
    return compile_program(X, items, "residual constraint conjuncts", servers, values, out, err);
}

// table_runner.cpp — the reference's table-driven StateMachine tests, run through the C++ host
// mirror (tb::StateMachine) on the GPU engine.
//
//   tb_table_runner <tests/golden/state_machine_tables.txt> [device]
//   tb_table_runner --query <prepares.bin> <answer.bin> [device]     (run_query below)
//   tb_table_runner --query-fields <transfers|accounts> <prepares.bin> <answer.bin> [device]
//
// The fixture holds the 18 check() tables of src/state_machine.zig:1531-2074 verbatim.  Row DSL:
// src/testing/table.zig:8-100 (tokens, `_` defaults, letter labels, `-N` = maxInt - N); action
// schema and harness: src/state_machine.zig:1247-1529 (TestAction, TestCreateAccount,
// TestCreateTransfer, check()).  Prints one line per table; exit status = number of failures.
#include <cctype>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "state_machine.hpp"

namespace {

using tb::u128;

struct ParseError : std::runtime_error {
    using std::runtime_error::runtime_error;
};

// table.zig:37-47: one leading letter is a label; `-N` on an unsigned field is maxInt - N.
u128 parse_int(const std::string& tok, int bits) {
    size_t i = (!tok.empty() && std::isalpha((unsigned char)tok[0])) ? 1 : 0;
    const u128 maxv = bits == 128 ? ~(u128)0 : (((u128)1 << bits) - 1);
    bool neg = false;
    if (i < tok.size() && tok[i] == '-') {
        neg = true;
        i++;
    }
    if (i >= tok.size()) throw ParseError("empty integer: " + tok);
    u128 v = 0;
    for (; i < tok.size(); i++) {
        if (!std::isdigit((unsigned char)tok[i])) throw ParseError("bad integer: " + tok);
        v = v * 10 + (u128)(tok[i] - '0');
    }
    if (neg) {
        if (v > maxv) throw ParseError("out of range: " + tok);
        return maxv - v;
    }
    if (v > maxv) throw ParseError("out of range: " + tok);
    return v;
}

struct Tokens {
    std::vector<std::string> t;
    size_t i = 0;
    bool more() const { return i < t.size(); }
    const std::string& peek() const { return t[i]; }
    std::string next() {
        if (i >= t.size()) throw ParseError("row too short");
        return t[i++];
    }
};

// A column: bits > 0 integer, bits == 0 flag (token), bits < 0 result enum.
struct Column {
    const char* name;
    int bits;
    const char* flag;
    bool required;
};

const Column kAccountColumns[] = {  // TestCreateAccount (state_machine.zig:1281-1298)
    {"id", 128, nullptr, true},          {"debits_pending", 128, nullptr, false},
    {"debits_posted", 128, nullptr, false}, {"credits_pending", 128, nullptr, false},
    {"credits_posted", 128, nullptr, false}, {"user_data_128", 128, nullptr, false},
    {"user_data_64", 64, nullptr, false}, {"user_data_32", 32, nullptr, false},
    {"reserved", 1, nullptr, false},     {"ledger", 32, nullptr, true},
    {"code", 16, nullptr, true},         {"linked", 0, "LNK", false},
    {"debits_must_not_exceed_credits", 0, "D<C", false},
    {"credits_must_not_exceed_debits", 0, "C<D", false},
    {"flags_padding", 13, nullptr, false}, {"timestamp", 64, nullptr, false},
    {"result", -1, nullptr, true},
};

const Column kTransferColumns[] = {  // TestCreateTransfer (state_machine.zig:1324-1344)
    {"id", 128, nullptr, true},          {"debit_account_id", 128, nullptr, true},
    {"credit_account_id", 128, nullptr, true}, {"amount", 128, nullptr, false},
    {"pending_id", 128, nullptr, false}, {"user_data_128", 128, nullptr, false},
    {"user_data_64", 64, nullptr, false}, {"user_data_32", 32, nullptr, false},
    {"timeout", 32, nullptr, false},     {"ledger", 32, nullptr, true},
    {"code", 16, nullptr, true},         {"linked", 0, "LNK", false},
    {"pending", 0, "PEN", false},        {"post_pending_transfer", 0, "POS", false},
    {"void_pending_transfer", 0, "VOI", false}, {"balancing_debit", 0, "BDR", false},
    {"balancing_credit", 0, "BCR", false}, {"flags_padding", 10, nullptr, false},
    {"timestamp", 64, nullptr, false},   {"result", -2, nullptr, true},
};

uint32_t result_index(const std::vector<std::string>& names, const std::string& tok) {
    for (size_t i = 0; i < names.size(); i++) {
        if (names[i] == tok) return (uint32_t)i;
    }
    throw ParseError("unknown result: " + tok);
}

// table.zig:49-71: `_` selects a field's default, only for fields that have one.
template <size_t N>
std::map<std::string, u128> parse_struct(Tokens& toks, const Column (&cols)[N]) {
    std::map<std::string, u128> row;
    for (const Column& c : cols) {
        if (!c.required && toks.more() && toks.peek() == "_") {
            toks.next();
            row[c.name] = 0;
            continue;
        }
        const std::string tok = toks.next();
        if (c.bits > 0) {
            row[c.name] = parse_int(tok, c.bits);
        } else if (c.bits == 0) {
            if (tok != c.flag) throw ParseError("unknown flag " + tok + " (expected " + c.flag + ")");
            row[c.name] = 1;
        } else {
            row[c.name] = result_index(c.bits == -1 ? tb::create_account_result_names() : tb::create_transfer_result_names(),
                                       tok);
        }
    }
    return row;
}

tb::Account account_event(std::map<std::string, u128>& r) {  // state_machine.zig:1300-1321
    tb::Account a{};
    a.id = r["id"];
    a.debits_pending = r["debits_pending"];
    a.debits_posted = r["debits_posted"];
    a.credits_pending = r["credits_pending"];
    a.credits_posted = r["credits_posted"];
    a.user_data_128 = r["user_data_128"];
    a.user_data_64 = (uint64_t)r["user_data_64"];
    a.user_data_32 = (uint32_t)r["user_data_32"];
    a.reserved = (uint32_t)r["reserved"];
    a.ledger = (uint32_t)r["ledger"];
    a.code = (uint16_t)r["code"];
    a.flags = (uint16_t)((r["linked"] ? tb::AccountFlags::linked : 0) |
                         (r["debits_must_not_exceed_credits"] ? tb::AccountFlags::debits_must_not_exceed_credits : 0) |
                         (r["credits_must_not_exceed_debits"] ? tb::AccountFlags::credits_must_not_exceed_debits : 0) |
                         ((uint16_t)r["flags_padding"] << 3));
    a.timestamp = (uint64_t)r["timestamp"];
    return a;
}

tb::Transfer transfer_event(std::map<std::string, u128>& r) {  // state_machine.zig:1346-1370
    tb::Transfer t{};
    t.id = r["id"];
    t.debit_account_id = r["debit_account_id"];
    t.credit_account_id = r["credit_account_id"];
    t.amount = r["amount"];
    t.pending_id = r["pending_id"];
    t.user_data_128 = r["user_data_128"];
    t.user_data_64 = (uint64_t)r["user_data_64"];
    t.user_data_32 = (uint32_t)r["user_data_32"];
    t.timeout = (uint32_t)r["timeout"];
    t.ledger = (uint32_t)r["ledger"];
    t.code = (uint16_t)r["code"];
    t.flags = (uint16_t)((r["linked"] ? tb::TransferFlags::linked : 0) | (r["pending"] ? tb::TransferFlags::pending : 0) |
                         (r["post_pending_transfer"] ? tb::TransferFlags::post_pending_transfer : 0) |
                         (r["void_pending_transfer"] ? tb::TransferFlags::void_pending_transfer : 0) |
                         (r["balancing_debit"] ? tb::TransferFlags::balancing_debit : 0) |
                         (r["balancing_credit"] ? tb::TransferFlags::balancing_credit : 0) |
                         ((uint16_t)r["flags_padding"] << 6));
    t.timestamp = (uint64_t)r["timestamp"];
    return t;
}

template <typename T>
void append(std::vector<uint8_t>& buf, const T& v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(&v);
    buf.insert(buf.end(), p, p + sizeof(T));
}

std::string describe(const std::vector<uint8_t>& b, bool creates) {
    std::ostringstream os;
    if (creates) {
        for (size_t i = 0; i + 8 <= b.size(); i += 8) {
            uint32_t idx, res;
            memcpy(&idx, &b[i], 4);
            memcpy(&res, &b[i + 4], 4);
            os << "(" << idx << "," << res << ")";
        }
    } else {
        os << b.size() / 128 << " records";
    }
    return os.str();
}

// check() (state_machine.zig:1373-1529) for one table.
std::string run_table(tb::StateMachine& sm, const std::string& text) {
    std::map<u128, tb::Account> accounts;
    std::map<u128, tb::Transfer> transfers;
    std::vector<uint8_t> request, reply;
    int operation = 0;  // 0 = none yet
    uint64_t prepare_timestamp = 0;
    std::vector<uint8_t> output(tb::message_body_size_max);
    uint64_t op_number = 0;

    std::istringstream lines(text);
    std::string line;
    while (std::getline(lines, line)) {
        Tokens toks;
        std::istringstream ls(line);
        for (std::string w; ls >> w;) toks.t.push_back(w);
        if (toks.t.empty()) continue;
        const std::string variant = toks.next();
        if (variant == "setup") {
            u128 v[5];
            for (u128& x : v) x = parse_int(toks.next(), 128);
            sm.test_set_balances(v[0], v[1], v[2], v[3], v[4]);
        } else if (variant == "tick") {
            prepare_timestamp += (uint64_t)parse_int(toks.next(), 64);
        } else if (variant == "account") {
            auto r = parse_struct(toks, kAccountColumns);
            operation = (int)tb::Operation::create_accounts;
            const tb::Account a = account_event(r);
            append(request, a);
            if (r["result"] == 0) accounts[a.id] = a;
            else append(reply, tb::CreateResult{(uint32_t)(request.size() / 128 - 1), (uint32_t)r["result"]});
        } else if (variant == "transfer") {
            auto r = parse_struct(toks, kTransferColumns);
            operation = (int)tb::Operation::create_transfers;
            const tb::Transfer t = transfer_event(r);
            append(request, t);
            if (r["result"] == 0) transfers[t.id] = t;
            else append(reply, tb::CreateResult{(uint32_t)(request.size() / 128 - 1), (uint32_t)r["result"]});
        } else if (variant == "lookup_account") {
            operation = (int)tb::Operation::lookup_accounts;
            const u128 id = parse_int(toks.next(), 128);
            append(request, id);
            if (toks.peek() == "_") {
                toks.next();
            } else {
                tb::Account a = accounts.at(id);
                a.debits_pending = parse_int(toks.next(), 128);
                a.debits_posted = parse_int(toks.next(), 128);
                a.credits_pending = parse_int(toks.next(), 128);
                a.credits_posted = parse_int(toks.next(), 128);
                append(reply, a);
            }
        } else if (variant == "lookup_transfer") {
            operation = (int)tb::Operation::lookup_transfers;
            const u128 id = parse_int(toks.next(), 128);
            append(request, id);
            const std::string kind = toks.next();
            if (kind == "exists") {
                const std::string v = toks.next();
                if (v == "true" || v == "T" || v == "1") append(reply, transfers.at(id));
            } else if (kind == "amount") {
                tb::Transfer t = transfers.at(id);
                t.amount = parse_int(toks.next(), 128);
                append(reply, t);
            } else {
                throw ParseError("unknown lookup_transfer variant " + kind);
            }
        } else if (variant == "commit") {
            const std::string name = toks.next();
            const tb::Operation op = name == "create_accounts"    ? tb::Operation::create_accounts
                                     : name == "create_transfers" ? tb::Operation::create_transfers
                                     : name == "lookup_accounts"  ? tb::Operation::lookup_accounts
                                     : name == "lookup_transfers" ? tb::Operation::lookup_transfers
                                                                  : throw ParseError("unknown operation " + name);
            if (operation != 0 && operation != (int)op) throw ParseError("commit of a different operation");
            prepare_timestamp += 1;
            sm.prepare_timestamp = prepare_timestamp;
            sm.prepare(op, request.data(), request.size());  // state_machine.zig:336-343
            prepare_timestamp = sm.prepare_timestamp;
            sm.prefetch([](tb::StateMachine&) {}, ++op_number, op, request.data(), request.size());
            size_t n = sm.commit(0, op_number, prepare_timestamp, op, request.data(), request.size(), output.data());
            std::vector<uint8_t> actual(output.begin(), output.begin() + n);
            const bool creates = op == tb::Operation::create_accounts || op == tb::Operation::create_transfers;
            if (!creates) {  // :1500-1506 lookups zero every returned timestamp
                for (size_t off = 0; off + 128 <= actual.size(); off += 128) memset(&actual[off + 120], 0, 8);
            }
            if (actual != reply) {
                return "reply mismatch for " + name + ": expected " + describe(reply, creates) + " got " +
                       describe(actual, creates);
            }
            request.clear();
            reply.clear();
            operation = 0;
        } else {
            throw ParseError("unknown row variant " + variant);
        }
        if (toks.more() && toks.peek() != "//") throw ParseError("trailing token " + toks.peek());
    }
    return "";
}

// --query: prepares then one account filter through tb::StateMachine, for tests/test_gpu_query_cpp.py
// to compare with the Python mirror's answer.  <prepares.bin>: {u64 timestamp, u32 operation, u32
// body bytes, body} per prepare, then {0, 0, 64, a tbgpu_account_filter}.  <answer.bin> receives the
// 16-byte tbgpu_query_result and the records.
// --query-fields (tests/test_gpu_query_filter_cpp.py): the same files, the prepares ending in a
// tbgpu_query_filter for query_transfers or query_accounts.
// --query-balances (tests/test_gpu_balances_cpp.py): --query's files, answered by get_account_balances
// (the records are tbgpu_account_balance rows).
// --query-change-events (tests/test_gpu_change_events_cpp.py): the prepares ending in a
// tbgpu_change_events_filter, answered by get_change_events (the records are 384-byte events).
// --query-many (tests/test_gpu_query_many_cpp.py): the prepares ending in {0, 0, n * 64, n
// tbgpu_account_filter}, answered by get_account_transfers_many; <answer.bin> receives, per filter,
// the 16-byte tbgpu_query_result and then its records.
// --query-accounts-at (tests/test_gpu_lookup_at_cpp.py): the prepares ending in {0, 0, 8 + n * 16, a u64
// timestamp and n ids}, answered by lookup_accounts_at (the records are accounts).
// --query-ledgers (tests/test_gpu_ledger_balances_cpp.py): the prepares ending in {0, 0, 8 + n * 4, a u64
// timestamp and n u32 ledgers}, answered by get_ledger_balances (the records are tbgpu_ledger_balance rows).
// --query-pending (tests/test_gpu_pending_cpp.py): the prepares ending in {0, 0, 64, a tbgpu_pending_filter},
// answered by get_pending_transfers: the result, the rows (tbgpu_pending_row) and then a state byte a row.
// --query-statements (tests/test_gpu_statements_cpp.py): the prepares ending in {0, 0, 16 + n * 16, t_open,
// t_close and n ids}, answered by get_account_statements (the records are tbgpu_account_statement rows).
// --query-integrals (tests/test_gpu_integrals_cpp.py): the same request, answered by
// get_account_balance_integrals (the records are tbgpu_account_balance_integral rows).
// --query-extremes (tests/test_gpu_extremes_cpp.py): the prepares ending in {0, 0, 24 + n * 16, t_open, t_close,
// the 8 bytes of a tbgpu_balance_measure and n ids}, answered by get_account_balance_extremes (the records are
// tbgpu_account_balance_extreme rows).
// --query-series (tests/test_gpu_series_cpp.py): the prepares ending in {0, 0, the body's length, u32 n_buckets,
// u32 n_ids, n_buckets + 1 bounds and n_ids ids}, answered by get_account_statement_series (the records are
// tbgpu_account_statement rows).
// --query-flow-matrix (tests/test_gpu_matrix_cpp.py): the prepares ending in {0, 0, the body's length, t_open,
// t_close, u32 n_debit, u32 n_credit, n_debit debit ids and n_credit credit ids}, answered by
// get_account_flow_matrix (the records are tbgpu_flow_cell cells).
// --query-counterparties (tests/test_gpu_counterparties_cpp.py): the prepares ending in {0, 0, 64, a
// tbgpu_counterparty_filter}, answered by get_account_counterparties (the records are tbgpu_counterparty rows).
// --query-active (tests/test_gpu_activity_cpp.py): the prepares ending in {0, 0, 64, a tbgpu_activity_filter},
// answered by get_active_accounts (the records are tbgpu_account_activity rows).
enum QueryKind { ACCOUNT_TRANSFERS, ACCOUNT_BALANCES, QUERY_TRANSFERS, QUERY_ACCOUNTS, CHANGE_EVENTS, ACCOUNT_TRANSFERS_MANY, ACCOUNTS_AT,
                 LEDGER_BALANCES, PENDING_TRANSFERS, ACCOUNT_STATEMENTS, ACCOUNT_INTEGRALS, ACCOUNT_SERIES, ACCOUNT_FLOW_MATRIX,
                 ACCOUNT_COUNTERPARTIES, ACTIVE_ACCOUNTS, ACCOUNT_EXTREMES };

int run_query(tb::StateMachine& sm, QueryKind kind, const char* in_path, const char* out_path) {
    std::ifstream in(in_path, std::ios::binary);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", in_path);
        return 2;
    }
    std::vector<uint8_t> body, reply;
    uint64_t op = 0;
    for (;;) {
        uint64_t ts = 0;
        uint32_t operation = 0, len = 0;
        in.read((char*)&ts, 8).read((char*)&operation, 4).read((char*)&len, 4);
        body.resize(len);
        if (!in || !in.read((char*)body.data(), len)) {
            fprintf(stderr, "%s: truncated\n", in_path);
            return 2;
        }
        if (operation == 0) break;
        reply.resize((size_t)len / 128 * 8 + 8);
        sm.commit(0, ++op, ts, (tb::Operation)operation, body.data(), body.size(), reply.data());
    }
    tbgpu_account_filter f;
    tbgpu_query_filter q;
    tbgpu_change_events_filter c;
    static_assert(sizeof(f) == sizeof(q) && sizeof(f) == sizeof(c), "every filter is 64 bytes");
    if (kind == ACCOUNT_TRANSFERS_MANY) {
        const size_t n = body.size() / sizeof(f);
        if (body.size() % sizeof(f) || n == 0 || n > TBGPU_QUERY_FILTERS_MAX) {
            fprintf(stderr, "%s: 1 to %u filters of %zu bytes\n", in_path, TBGPU_QUERY_FILTERS_MAX, sizeof(f));
            return 2;
        }
        std::vector<tbgpu_account_filter> filters(n);
        memcpy(filters.data(), body.data(), body.size());
        std::vector<tbgpu_query_result> results(n);
        std::vector<uint8_t> out(n * (size_t)TBGPU_BATCH_EVENTS_MAX * 128);
        sm.get_account_transfers_many(filters.data(), (uint32_t)n, out.data(), TBGPU_BATCH_EVENTS_MAX, results.data());
        std::ofstream o(out_path, std::ios::binary);
        for (size_t i = 0; i < n; i++) {
            o.write((const char*)&results[i], sizeof(results[i]))
                .write((const char*)out.data() + i * (size_t)TBGPU_BATCH_EVENTS_MAX * 128, (size_t)results[i].count * 128);
            printf("query %zu: %u of %llu records, complete %u\n", i, results[i].count, (unsigned long long)results[i].matched,
                   results[i].complete);
        }
        return o ? 0 : 2;
    }
    if (kind == ACCOUNTS_AT) {
        const size_t n = body.size() / 16;
        if (body.size() % 16 != 8 || n > TBGPU_LOOKUP_AT_MAX) {
            fprintf(stderr, "%s: a timestamp and at most %u ids of 16 bytes\n", in_path, TBGPU_LOOKUP_AT_MAX);
            return 2;
        }
        uint64_t timestamp = 0;
        memcpy(&timestamp, body.data(), 8);
        std::vector<uint8_t> out((size_t)TBGPU_LOOKUP_AT_MAX * 128);
        const tbgpu_query_result r = sm.lookup_accounts_at(timestamp, body.data() + 8, (uint32_t)n, out.data(), TBGPU_LOOKUP_AT_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * 128);
        printf("query: %u of %llu records, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (kind == LEDGER_BALANCES) {
        const size_t n = body.size() / 4 - 2;
        if (body.size() < 8 || body.size() % 4 || n > TBGPU_LEDGERS_MAX) {
            fprintf(stderr, "%s: a timestamp and at most %u ledgers of 4 bytes\n", in_path, TBGPU_LEDGERS_MAX);
            return 2;
        }
        uint64_t timestamp = 0;
        memcpy(&timestamp, body.data(), 8);
        std::vector<uint32_t> ledgers(n);
        memcpy(ledgers.data(), body.data() + 8, n * 4);
        std::vector<uint8_t> out((size_t)TBGPU_LEDGERS_MAX * sizeof(tbgpu_ledger_balance));
        const tbgpu_query_result r = sm.get_ledger_balances(timestamp, ledgers.data(), (uint32_t)n, out.data(), TBGPU_LEDGERS_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * sizeof(tbgpu_ledger_balance));
        printf("query: %u of %llu rows, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (kind == ACCOUNT_STATEMENTS) {
        const size_t n = body.size() >= 16 ? body.size() / 16 - 1 : 0;
        if (body.size() % 16 != 0 || body.size() < 16 || n > TBGPU_STATEMENTS_MAX) {
            fprintf(stderr, "%s: t_open, t_close and at most %u ids of 16 bytes\n", in_path, TBGPU_STATEMENTS_MAX);
            return 2;
        }
        uint64_t period[2] = {0, 0};
        memcpy(period, body.data(), 16);
        std::vector<uint8_t> out((size_t)TBGPU_STATEMENTS_MAX * sizeof(tbgpu_account_statement));
        const tbgpu_query_result r =
            sm.get_account_statements(period[0], period[1], body.data() + 16, (uint32_t)n, out.data(), TBGPU_STATEMENTS_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * sizeof(tbgpu_account_statement));
        printf("query: %u of %llu rows, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (kind == ACCOUNT_INTEGRALS) {
        const size_t n = body.size() >= 16 ? body.size() / 16 - 1 : 0;
        if (body.size() % 16 != 0 || body.size() < 16 || n > TBGPU_INTEGRALS_MAX) {
            fprintf(stderr, "%s: t_open, t_close and at most %u ids of 16 bytes\n", in_path, TBGPU_INTEGRALS_MAX);
            return 2;
        }
        uint64_t period[2] = {0, 0};
        memcpy(period, body.data(), 16);
        std::vector<uint8_t> out((size_t)TBGPU_INTEGRALS_MAX * sizeof(tbgpu_account_balance_integral));
        const tbgpu_query_result r =
            sm.get_account_balance_integrals(period[0], period[1], body.data() + 16, (uint32_t)n, out.data(), TBGPU_INTEGRALS_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * sizeof(tbgpu_account_balance_integral));
        printf("query: %u of %llu rows, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (kind == ACCOUNT_EXTREMES) {
        const size_t n = body.size() >= 24 ? (body.size() - 24) / 16 : 0;
        if (body.size() % 16 != 8 || body.size() < 24 || n > TBGPU_EXTREMES_MAX) {
            fprintf(stderr, "%s: t_open, t_close, a measure of 8 bytes and at most %u ids of 16 bytes\n", in_path, TBGPU_EXTREMES_MAX);
            return 2;
        }
        uint64_t period[2] = {0, 0};
        tbgpu_balance_measure measure;
        memcpy(period, body.data(), 16);
        memcpy(&measure, body.data() + 16, 8);
        std::vector<uint8_t> out((size_t)TBGPU_EXTREMES_MAX * sizeof(tbgpu_account_balance_extreme));
        const tbgpu_query_result r =
            sm.get_account_balance_extremes(period[0], period[1], measure, body.data() + 24, (uint32_t)n, out.data(), TBGPU_EXTREMES_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * sizeof(tbgpu_account_balance_extreme));
        printf("query: %u of %llu rows, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (kind == ACCOUNT_SERIES) {
        uint32_t head[2] = {0, 0};  // n_buckets, n_ids
        if (body.size() >= 8) memcpy(head, body.data(), 8);
        const size_t bounds_bytes = ((size_t)head[0] + 1) * 8;
        if (body.size() < 8 || head[0] == 0 || (uint64_t)head[0] * head[1] > TBGPU_SERIES_ROWS_MAX ||
            body.size() != 8 + bounds_bytes + (size_t)head[1] * 16) {
            fprintf(stderr, "%s: n_buckets, n_ids, n_buckets + 1 bounds and the ids of 16 bytes, at most %u rows\n", in_path,
                    TBGPU_SERIES_ROWS_MAX);
            return 2;
        }
        std::vector<uint64_t> bounds((size_t)head[0] + 1);
        memcpy(bounds.data(), body.data() + 8, bounds_bytes);
        std::vector<uint8_t> out((size_t)TBGPU_SERIES_ROWS_MAX * sizeof(tbgpu_account_statement));
        const tbgpu_query_result r = sm.get_account_statement_series(bounds.data(), head[0], body.data() + 8 + bounds_bytes, head[1],
                                                                     out.data(), TBGPU_SERIES_ROWS_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * sizeof(tbgpu_account_statement));
        printf("query: %u of %llu rows, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (kind == ACCOUNT_FLOW_MATRIX) {
        uint64_t period[2] = {0, 0};
        uint32_t head[2] = {0, 0};  // n_debit, n_credit
        if (body.size() >= 24) memcpy(period, body.data(), 16), memcpy(head, body.data() + 16, 8);
        if (body.size() < 24 || (uint64_t)head[0] * head[1] > TBGPU_FLOW_MATRIX_CELLS_MAX ||
            body.size() != 24 + ((size_t)head[0] + head[1]) * 16) {
            fprintf(stderr, "%s: t_open, t_close, n_debit, n_credit and the ids of 16 bytes, at most %u cells\n", in_path,
                    TBGPU_FLOW_MATRIX_CELLS_MAX);
            return 2;
        }
        std::vector<uint8_t> out((size_t)TBGPU_FLOW_MATRIX_CELLS_MAX * sizeof(tbgpu_flow_cell));
        const tbgpu_query_result r = sm.get_account_flow_matrix(period[0], period[1], body.data() + 24, head[0],
                                                                body.data() + 24 + (size_t)head[0] * 16, head[1], out.data(),
                                                                TBGPU_FLOW_MATRIX_CELLS_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * sizeof(tbgpu_flow_cell));
        printf("query: %u of %llu cells, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (kind == ACCOUNT_COUNTERPARTIES) {
        tbgpu_counterparty_filter cf;
        if (body.size() != sizeof(cf)) {
            fprintf(stderr, "%s: a counterparty filter is %zu bytes\n", in_path, sizeof(cf));
            return 2;
        }
        memcpy(&cf, body.data(), sizeof(cf));
        std::vector<uint8_t> out((size_t)TBGPU_COUNTERPARTIES_ROWS_MAX * sizeof(tbgpu_counterparty));
        const tbgpu_query_result r = sm.get_account_counterparties(cf, out.data(), TBGPU_COUNTERPARTIES_ROWS_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * sizeof(tbgpu_counterparty));
        printf("query: %u of %llu rows, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (kind == ACTIVE_ACCOUNTS) {
        tbgpu_activity_filter af;
        if (body.size() != sizeof(af)) {
            fprintf(stderr, "%s: an activity filter is %zu bytes\n", in_path, sizeof(af));
            return 2;
        }
        memcpy(&af, body.data(), sizeof(af));
        std::vector<uint8_t> out((size_t)TBGPU_ACTIVE_ROWS_MAX * sizeof(tbgpu_account_activity));
        const tbgpu_query_result r = sm.get_active_accounts(af, out.data(), TBGPU_ACTIVE_ROWS_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * sizeof(tbgpu_account_activity));
        printf("query: %u of %llu rows, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (kind == PENDING_TRANSFERS) {
        tbgpu_pending_filter pf;
        if (body.size() != sizeof(pf)) {
            fprintf(stderr, "%s: a pending filter is %zu bytes\n", in_path, sizeof(pf));
            return 2;
        }
        memcpy(&pf, body.data(), sizeof(pf));
        std::vector<uint8_t> rows((size_t)TBGPU_PENDING_ROWS_MAX * sizeof(tbgpu_pending_row)), states(TBGPU_PENDING_ROWS_MAX);
        const tbgpu_query_result r = sm.get_pending_transfers(pf, rows.data(), states.data(), TBGPU_PENDING_ROWS_MAX);
        std::ofstream o(out_path, std::ios::binary);
        o.write((const char*)&r, sizeof(r)).write((const char*)rows.data(), (size_t)r.count * sizeof(tbgpu_pending_row));
        o.write((const char*)states.data(), r.count);
        printf("query: %u of %llu rows, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
        return o ? 0 : 2;
    }
    if (body.size() != sizeof(f)) {
        fprintf(stderr, "%s: a filter is %zu bytes\n", in_path, sizeof(f));
        return 2;
    }
    memcpy(&f, body.data(), sizeof(f));
    memcpy(&q, body.data(), sizeof(q));
    memcpy(&c, body.data(), sizeof(c));
    std::vector<uint8_t> out((size_t)TBGPU_BATCH_EVENTS_MAX * 128);
    const size_t record = kind == CHANGE_EVENTS ? sizeof(tbgpu_change_event) : 128;
    const tbgpu_query_result r = kind == CHANGE_EVENTS ? sm.get_change_events(c, out.data(), TBGPU_CHANGE_EVENTS_MAX)
                                 : kind == ACCOUNT_TRANSFERS ? sm.get_account_transfers(f, out.data(), TBGPU_BATCH_EVENTS_MAX)
                                 : kind == ACCOUNT_BALANCES ? sm.get_account_balances(f, out.data(), TBGPU_BATCH_EVENTS_MAX)
                                 : kind == QUERY_TRANSFERS ? sm.query_transfers(q, out.data(), TBGPU_BATCH_EVENTS_MAX)
                                                           : sm.query_accounts(q, out.data(), TBGPU_BATCH_EVENTS_MAX);
    std::ofstream o(out_path, std::ios::binary);
    o.write((const char*)&r, sizeof(r)).write((const char*)out.data(), (size_t)r.count * record);
    printf("query: %u of %llu records, complete %u\n", r.count, (unsigned long long)r.matched, r.complete);
    return o ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
    const bool fields = argc > 1 && std::string(argv[1]) == "--query-fields";
    const bool balances = argc > 1 && std::string(argv[1]) == "--query-balances";
    const bool changes = argc > 1 && std::string(argv[1]) == "--query-change-events";
    const bool many = argc > 1 && std::string(argv[1]) == "--query-many";
    const bool at = argc > 1 && std::string(argv[1]) == "--query-accounts-at";
    const bool ledgers = argc > 1 && std::string(argv[1]) == "--query-ledgers";
    const bool pending = argc > 1 && std::string(argv[1]) == "--query-pending";
    const bool statements = argc > 1 && std::string(argv[1]) == "--query-statements";
    const bool integrals = argc > 1 && std::string(argv[1]) == "--query-integrals";
    const bool extremes = argc > 1 && std::string(argv[1]) == "--query-extremes";
    const bool series = argc > 1 && std::string(argv[1]) == "--query-series";
    const bool matrix = argc > 1 && std::string(argv[1]) == "--query-flow-matrix";
    const bool counterparties = argc > 1 && std::string(argv[1]) == "--query-counterparties";
    const bool active = argc > 1 && std::string(argv[1]) == "--query-active";
    const bool query = active || counterparties || matrix || fields || balances || changes || many || at || ledgers || pending || statements || integrals || extremes || series || (argc > 1 && std::string(argv[1]) == "--query");
    QueryKind kind = extremes ? ACCOUNT_EXTREMES : active ? ACTIVE_ACCOUNTS : counterparties ? ACCOUNT_COUNTERPARTIES : matrix ? ACCOUNT_FLOW_MATRIX : series ? ACCOUNT_SERIES : balances ? ACCOUNT_BALANCES : changes ? CHANGE_EVENTS : many ? ACCOUNT_TRANSFERS_MANY : at ? ACCOUNTS_AT : ledgers ? LEDGER_BALANCES : pending ? PENDING_TRANSFERS : statements ? ACCOUNT_STATEMENTS : integrals ? ACCOUNT_INTEGRALS : ACCOUNT_TRANSFERS;
    const char* self = argv[0];
    if (fields && argc > 2) {
        const std::string which = argv[2];
        kind = which == "transfers" ? QUERY_TRANSFERS : QUERY_ACCOUNTS;
        if (which != "transfers" && which != "accounts") argc = 0;  // usage
        argv++, argc--;  // the paths and the device now sit where --query has them
    }
    if (argc < 2 || (query && argc < 4)) {
        fprintf(stderr,
                "usage: %s <state_machine_tables.txt> [device]\n       %s --query <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-many <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-balances <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-change-events <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-accounts-at <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-ledgers <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-pending <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-statements <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-integrals <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-extremes <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-series <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-flow-matrix <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-counterparties <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-active <prepares.bin> <answer.bin> [device]\n"
                "       %s --query-fields <transfers|accounts> <prepares.bin> <answer.bin> [device]\n",
                self, self, self, self, self, self, self, self, self, self, self, self, self, self, self, self);
        return 2;
    }
    if (query) {
        tb::Options o;
        o.accounts_max = 4096;
        o.transfers_max = 1 << 14;
        o.pass_events_max = 8192 * 4;
        o.pass_batches_max = 64;
        o.device = argc > 4 ? atoi(argv[4]) : 0;
        try {
            tb::StateMachine sm(o);
            return run_query(sm, kind, argv[2], argv[3]);
        } catch (const std::exception& e) {
            fprintf(stderr, "query failed: %s\n", e.what());
            return 255;
        }
    }
    std::ifstream in(argv[1]);
    if (!in) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    tb::Options o;
    o.accounts_max = 4096;
    o.transfers_max = 1 << 14;
    o.pass_events_max = 8192 * 4;
    o.pass_batches_max = 64;
    o.device = argc > 2 ? atoi(argv[2]) : 0;
    std::unique_ptr<tb::StateMachine> owner;
    try {
        owner.reset(new tb::StateMachine(o));  // StateMachine.init: the only fallible call
    } catch (const std::exception& e) {
        fprintf(stderr, "init failed: %s\n", e.what());
        return 255;
    }
    tb::StateMachine& sm = *owner;

    // Fixture: `@table <name>` ... `@end` blocks (tests/golden/extract_tables.py).
    int failures = 0, tables = 0;
    std::string line, name, body;
    bool inside = false;
    while (std::getline(in, line)) {
        if (line.rfind("@table ", 0) == 0) {
            name = line.substr(7);
            body.clear();
            inside = true;
        } else if (line == "@end" && inside) {
            inside = false;
            tables++;
            std::string err;
            try {
                sm.reset();
                err = run_table(sm, body);
            } catch (const tb::Panic& e) {
                err = std::string("panic: ") + e.what();
            } catch (const std::exception& e) {
                err = std::string("error: ") + e.what();
            }
            if (err.empty()) {
                printf("ok   %s\n", name.c_str());
            } else {
                printf("FAIL %s: %s\n", name.c_str(), err.c_str());
                failures++;
            }
        } else if (inside) {
            body += line + "\n";
        }
    }
    printf("%d tables, %d failed\n", tables, failures);
    return failures;
}

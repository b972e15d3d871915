// REFERENCE SHIM — TEST INFRASTRUCTURE ONLY.  The part of roscpp that the reference's FootholdPlanner touches, written
// from its usage: a parameter table the driver fills, member callbacks kept so the driver can deliver a map and call the
// service the way ROS would, publishers that keep what was published, logging that writes nothing (ROS_ERROR keeps its format string).
#pragma once
#include <any>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <iomanip>
#include <iostream>
#include <map>
#include <memory>
#include <mutex>
#include <sstream>
#include <stdexcept>
#include <string>
#include <vector>

#define ROS_SHIM_NOP(...) do { } while (0)
#define ROS_INFO(...) ROS_SHIM_NOP()
#define ROS_WARN(...) ROS_SHIM_NOP()
#define ROS_ERROR(...) ::ros::shimError(__VA_ARGS__)
#define ROS_DEBUG(...) ROS_SHIM_NOP()
#define ROS_FATAL(...) ROS_SHIM_NOP()
#define ROS_INFO_STREAM(args) ROS_SHIM_NOP()
#define ROS_WARN_STREAM(args) ROS_SHIM_NOP()
#define ROS_ERROR_STREAM(args) ROS_SHIM_NOP()
#define ROS_DEBUG_STREAM(args) ROS_SHIM_NOP()

namespace ros {

// rosout stand-in: nothing is written; the format strings of ROS_ERROR calls are kept (the reference reports some
// outcomes — a failed getSubmap, cpp:1629 — through the log alone).  Called from the reference's worker threads too.
inline std::mutex& shimErrorMutex() {
    static std::mutex m;
    return m;
}
inline std::vector<std::string>& shimErrors() {
    static std::vector<std::string> v;
    return v;
}
template <class... A>
inline void shimError(const char* fmt, A&&...) {
    std::lock_guard<std::mutex> lock(shimErrorMutex());
    shimErrors().emplace_back(fmt);
}

struct Time {
    double sec = 0.0;
    static Time now() { return Time(); }  // no clock: results must not depend on it
};
struct Duration {
    double sec = 0.0;
    Duration() = default;
    Duration(double s) : sec(s) {}
};

// Every message published on one topic, in order (back() is the last one).
struct TopicLog {
    std::vector<std::any> messages;
};

class Publisher {
public:
    Publisher() = default;
    explicit Publisher(std::shared_ptr<TopicLog> log) : log_(std::move(log)) {}
    template <class M>
    void publish(const M& m) const {
        if (log_) log_->messages.emplace_back(m);
    }

private:
    std::shared_ptr<TopicLog> log_;
};
class Subscriber {};
class ServiceServer {};

class NodeHandle {
public:
    // ---- the driver's side -------------------------------------------------------------------------
    void setParam(const std::string& key, double v) { num_[key] = v; }
    void setParam(const std::string& key, const std::string& v) { str_[key] = v; }
    template <class M>
    void deliver(const std::string& topic, const M& msg) {
        std::any_cast<std::function<void(M)>&>(subs_.at(topic))(msg);
    }
    template <class Req, class Res>
    bool call(const std::string& service, Req& req, Res& res) {
        return std::any_cast<std::function<bool(Req&, Res&)>&>(services_.at(service))(req, res);
    }
    const TopicLog& topic(const std::string& name) const {
        static const TopicLog empty;
        auto it = topics_.find(name);
        return it == topics_.end() ? empty : *it->second;
    }
    template <class M>
    std::vector<M> published(const std::string& name) const {
        std::vector<M> out;
        for (const std::any& a : topic(name).messages) out.push_back(std::any_cast<const M&>(a));
        return out;
    }

    // ---- what the reference calls --------------------------------------------------------------------
    template <class T>
    bool param(const std::string& key, T& value, const T& fallback) const {
        auto it = num_.find(key);
        if (it == num_.end()) {
            value = fallback;
            return false;
        }
        value = static_cast<T>(it->second);
        return true;
    }
    bool param(const std::string& key, std::string& value, const std::string& fallback) const {
        auto it = str_.find(key);
        value = it == str_.end() ? fallback : it->second;
        return it != str_.end();
    }
    template <class M, class T>
    Subscriber subscribe(const std::string& topic, uint32_t, void (T::*fp)(M), T* obj) {
        subs_[topic] = std::function<void(M)>([obj, fp](M m) { (obj->*fp)(m); });
        return Subscriber();
    }
    template <class M>
    Publisher advertise(const std::string& topic, uint32_t, bool = false) {
        auto& log = topics_[topic];
        if (!log) log = std::make_shared<TopicLog>();
        return Publisher(log);
    }
    template <class T, class Req, class Res>
    ServiceServer advertiseService(const std::string& service, bool (T::*fp)(Req&, Res&), T* obj) {
        services_[service] = std::function<bool(Req&, Res&)>([obj, fp](Req& a, Res& b) { return (obj->*fp)(a, b); });
        return ServiceServer();
    }
    void shutdown() {}

private:
    std::map<std::string, double> num_;
    std::map<std::string, std::string> str_;
    std::map<std::string, std::any> subs_, services_;
    std::map<std::string, std::shared_ptr<TopicLog>> topics_;
};

}  // namespace ros
